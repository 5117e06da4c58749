// anerf_kernels_small.hpp — the small __global__ kernels of anerf_render.hip: near/far + NaN fill, ray generation,
// the render call's per-ray stages (composite, importance sampling), composition, encoding stage.  Not templates, so one unit defines them (anerf_render_f16.hip includes
// anerf_kernels.hpp without this file).
#pragma once

// ======================================================================= small kernels
// ANERF_FLAG_NEAR_FAR: the caller's filled near / far (ray_batch columns 6, 7) into the workspace
__global__ void near_far_given_kernel(const float* __restrict__ rb, int stride, int64_t n, float* __restrict__ near_out,
                                      float* __restrict__ far_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    near_out[i] = rb[i * stride + 6];
    far_out[i] = rb[i * stride + 7];
}

__global__ void near_far_kernel(const float* __restrict__ rb, int stride, int64_t n, const float* __restrict__ cyls,
                                const int32_t* __restrict__ ray_pose, int n_poses, float* __restrict__ near_out,
                                float* __restrict__ far_out, uint8_t* __restrict__ qnan) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* r = rb + i * stride;
    const int pose = ray_pose ? ray_pose[i] : 0;
    if (pose < 0 || pose >= n_poses) {  // out-of-range pose index: a miss (filled by the chunk mean)
        near_out[i] = far_out[i] = __int_as_float(0x7fc00000);
        qnan[i] = 1;
        return;
    }
    const float* cy = cyls + 5 * pose;
    const float nearv = r[6], farv = r[7];
    // g_axes = [0, -1]: the x-z ground plane (ray_utils.py:292-327)
    const float rn0 = r[0] + r[3] * nearv, rn1 = r[2] + r[5] * nearv;
    const float rf0 = r[0] + r[3] * farv, rf1 = r[2] + r[5] * farv;
    const float nc0 = cy[0] - rn0, nc1 = cy[1] - rn1;
    const float nf0 = rf0 - rn0, nf1 = rf1 - rn1;
    const float nfn = norm2(nf0, nf1);
    const float scale = norm2(r[3], r[5]);
    const float cross = nc0 * nf1 - nc1 * nf0;
    const float dist = fabsf(cross) / nfn;
    const float rad = cy[2];
    const float Q = sqrtf(rad * rad - dist * dist);
    const float K = (nc0 * nf0 + nc1 * nf1) / nfn;
    const float mask = (Q < K) ? 1.0f : 0.0f;
    near_out[i] = nearv + (mask * (K - Q)) / scale;
    far_out[i] = nearv + (K + Q) / scale;
    qnan[i] = (Q != Q) ? 1 : 0;
}

// one workgroup per chunk: NaN rows <- np.nanmean of the chunk (ray_utils.py:328-342)
constexpr int NF_LEAVES = 1024;  // leaves of <= 128 rays: chunks up to ~65 k rays in parallel
constexpr int NF_LDS = 8192;     // chunks up to this many rays sum from LDS

__global__ void nan_fill_kernel(const float* __restrict__ rb, int stride, int64_t n, int chunk,
                                float* __restrict__ near_io, float* __restrict__ far_io,
                                const uint8_t* __restrict__ qnan, float* __restrict__ scratch) {
    const int64_t c0 = (int64_t)blockIdx.x * chunk;
    const int64_t c1 = min(c0 + chunk, n);
    const int64_t m = c1 - c0;
    __shared__ int any, n_leaves, valid[2];
    __shared__ float means[2];
    __shared__ int leaf_off[NF_LEAVES], leaf_cnt[NF_LEAVES];
    __shared__ float leaf_sum[NF_LEAVES];
    if (threadIdx.x == 0) { any = 0; valid[0] = valid[1] = 0; }
    __syncthreads();
    for (int64_t i = c0 + threadIdx.x; i < c1; i += blockDim.x)
        if (near_io[i] != near_io[i]) any = 1;
    __syncthreads();
    if (!any) return;
    __shared__ int st_a[64], st_b[64];  // (the tree walks' stacks, thread 0)
    __shared__ float st_v[64];
    if (threadIdx.x == 0) n_leaves = np_pairwise_leaves(m, leaf_off, leaf_cnt, NF_LEAVES, st_a, st_b);
    // NaN -> 0 copies, one vector at a time: in LDS for chunks up to NF_LDS rays (the leaf sums' loads then wait
    // on LDS, not on L2: 55 -> a few us for a 2048-ray training batch), else in the scratch
    __shared__ float lbuf[NF_LDS];
    float* buf = m <= NF_LDS ? lbuf : scratch + c0;
    for (int v = 0; v < 2; ++v) {
        const float* src = v == 0 ? near_io : far_io;
        int mine = 0;
        for (int64_t i = c0 + threadIdx.x; i < c1; i += blockDim.x) {
            const float x = src[i];
            buf[i - c0] = (x != x) ? 0.0f : x;
            mine += (x == x);
        }
        atomicAdd(&valid[v], mine);
        __syncthreads();
        // numpy's pairwise sum (np.nanmean, ray_utils.py:332): leaves in parallel, then the tree
        if (n_leaves >= 0)
            for (int k = threadIdx.x; k < n_leaves; k += blockDim.x) leaf_sum[k] = np_leaf_sum(buf + leaf_off[k], leaf_cnt[k]);
        __syncthreads();
        if (threadIdx.x == 0) {
            const float sum = n_leaves >= 0 ? np_pairwise_combine(leaf_sum, m, st_a, st_b, st_v) : np_pairwise_sum(buf, m);
            means[v] = valid[v] ? (float)((double)sum / (double)valid[v]) : __int_as_float(0x7fc00000);
        }
        __syncthreads();
    }
    for (int64_t i = c0 + threadIdx.x; i < c1; i += blockDim.x) {
        if (qnan[i]) {
            const float* r = rb + i * stride;
            near_io[i] = (means[0] != means[0]) ? r[6] : means[0];
            far_io[i] = (means[1] != means[1]) ? r[7] : means[1];
        }
    }
}

// ======================================================================= per-ray stages of the render call
// What follows a render_kernel launch (anerf_kernels.hpp), which ends at the raws in the workspace: raw2outputs and,
// after the coarse launch, the importance sampling -- composite() and importance() of anerf_stages.hpp, the functions
// render_fused_kernel runs in the kernel, on the same values in the same order.  Their transmittance product and cdf
// sum are sequential double-precision chains on lane 0: here one wave per ray in 64-thread workgroups with a few KB of
// LDS each, so a CU holds dozens of rays and the chains' latency is hidden (the render kernel is one wave per SIMD).
// LDS: ray slot [16] (composite reads |d| at 9), z [zs], (coarse: zf [zs],) scratch [8 zs] as render_item's
// (composite's w, wz, wc, fac, al, importance's scratch from zs on, the results at 7 zs); zs = pad32(S + I).
__host__ __device__ inline int render_stage_lds_floats(int S, int I, bool coarse) {
    return 16 + ((coarse && I > 0) ? 10 : 9) * pad32(S + I);
}

__device__ __forceinline__ void render_stage_maps(const float* res, int lane, int64_t i, float* __restrict__ o_rgb,
                                                  float* __restrict__ o_disp, float* __restrict__ o_acc) {
    if (lane < 5) {
        const float v = res[lane];
        if (lane < 3) {
            if (o_rgb) o_rgb[3 * i + lane] = v;
        } else if (lane == 3) {
            if (o_disp) o_disp[i] = v;
        } else if (o_acc) {
            o_acc[i] = v;
        }
    }
}

// After the coarse launch: the coarse maps (the final ones when I == 0), alpha0, the coarse debug arrays, and the
// sorted fine z into A.zf_ws for the fine launch.  The z list is rebuilt from near / far exactly as render_item does.
__global__ __launch_bounds__(64) void render_coarse_stage_kernel(ModelDev M, RenderArgs A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int64_t i = blockIdx.x;
    const int lane = threadIdx.x, S = A.S, I = A.I, T = S + I;
    const int zs = pad32(T);
    float* ray = lds;
    float* z = lds + 16;
    float* zf = z + zs;  // (I > 0 only)
    float* scr = I > 0 ? zf + zs : zf;
    const float* src = A.rb + i * A.stride;
    if (lane == 0) ray[9] = norm3(src[3], src[4], src[5]);
    const float nearv = A.near[i], farv = A.far[i];
    for (int s = lane; s < S; s += 64) z[s] = lineseg_z(nearv, farv, torch_linspace01(s, S), A.lindisp != 0);
    wave_sync();
    const float* raw = A.raw_ws + i * S * 4;
    const bool final_pass = I == 0;
    float* o_alpha = final_pass ? A.alpha : A.alpha0;
    for (int s = lane; s < S; s += 64) {
        if (A.dbg_z0) A.dbg_z0[i * S + s] = z[s];
        if (A.dbg_raw0)
            for (int c = 0; c < 4; ++c) A.dbg_raw0[(i * S + s) * 4 + c] = raw[4 * s + c];
    }
    float* res = scr + 7 * zs;
    composite(M, ray, z, raw, S, scr, zs, true, lane, o_alpha ? o_alpha + i * S : nullptr, res);
    render_stage_maps(res, lane, i, final_pass ? A.rgb : A.rgb0, final_pass ? A.disp : A.disp0,
                      final_pass ? A.acc : A.acc0);
    if (I > 0) {
        if (A.dbg_w0)
            for (int s = lane; s < S; s += 64) A.dbg_w0[i * S + s] = scr[s];
        // (inlined at this call: as a call, the callee's register budget makes this a 280-register kernel with
        // scratch, one wave per SIMD -- the occupancy these kernels exist for)
        [[clang::always_inline]] importance(z, scr, S, I, zf, scr + zs, true, lane);
        for (int s = lane; s < T; s += 64) A.zf_ws[i * T + s] = zf[s];
    }
}

// After the fine launch: the final maps, alpha and the fine debug arrays from A.zf_ws and the fine raws.
__global__ __launch_bounds__(64) void render_fine_stage_kernel(ModelDev M, RenderArgs A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int64_t i = blockIdx.x;
    const int lane = threadIdx.x, T = A.S + A.I;
    const int zs = pad32(T);
    float* ray = lds;
    float* z = lds + 16;
    float* scr = z + zs;
    const float* src = A.rb + i * A.stride;
    if (lane == 0) ray[9] = norm3(src[3], src[4], src[5]);
    for (int s = lane; s < T; s += 64) z[s] = A.zf_ws[i * T + s];
    wave_sync();
    const float* raw = A.raw_ws + i * T * 4;
    for (int s = lane; s < T; s += 64) {
        if (A.dbg_z1) A.dbg_z1[i * T + s] = z[s];
        if (A.dbg_raw1)
            for (int c = 0; c < 4; ++c) A.dbg_raw1[(i * T + s) * 4 + c] = raw[4 * s + c];
    }
    float* res = scr + 7 * zs;
    composite(M, ray, z, raw, T, scr, zs, true, lane, A.alpha ? A.alpha + i * T : nullptr, res);
    render_stage_maps(res, lane, i, A.rgb, A.disp, A.acc);
}

// A frame's traced pixels: an explicit index list, or (idx == NULL) the row-major half-open box
// [x0, x0 + bw) x [y0, ...) of kp_to_valid_rays (ray_utils.py:127-130) generated on the fly.
struct PixelSet {
    const int64_t* idx;
    int64_t x0, y0, bw;
    __device__ __forceinline__ int64_t pixel(int64_t t, int W) const {
        return idx ? idx[t] : (y0 + t / bw) * W + x0 + t % bw;
    }
};

__global__ void gen_rays_kernel(const float* __restrict__ c2w, int H, int W, float fx, float fy, float cx, float cy,
                                PixelSet px, int64_t n, float nearv, float farv, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int64_t p = px.pixel(t, W);
    const float x = (float)(p % W), y = (float)(p / W);
    // dirs = ((i - cx)/fx, -(j - cy)/fy, -1); rays_d = sum(dirs * c2w[:3,:3], -1) (ray_utils.py:22-25)
    const float d0 = (x - cx) / fx;
    const float d1 = -(y - cy) / fy;
    const float d2 = -1.0f;
    float* o = out + t * 11;
    float dd[3];
    for (int r = 0; r < 3; ++r) {
        dd[r] = (d0 * c2w[4 * r + 0] + d1 * c2w[4 * r + 1]) + d2 * c2w[4 * r + 2];
        o[r] = c2w[4 * r + 3];
        o[3 + r] = dd[r];
    }
    o[6] = nearv;
    o[7] = farv;
    const float nn = norm3(dd[0], dd[1], dd[2]);  // viewdirs = d / |d| (core/trainer.py:123)
    o[8] = dd[0] / nn;
    o[9] = dd[1] / nn;
    o[10] = dd[2] / nn;
}

__global__ void compose_fill_kernel(const float* __restrict__ bg, int white, int64_t hw, float* __restrict__ out_rgb,
                                    float* __restrict__ out_disp, float* __restrict__ out_acc) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= hw) return;
    for (int c = 0; c < 3; ++c) out_rgb[3 * p + c] = bg ? bg[3 * p + c] : (white ? 1.0f : 0.0f);
    out_disp[p] = 0.0f;
    if (out_acc) out_acc[p] = 0.0f;
}

__global__ void compose_scatter_kernel(const float* __restrict__ rgb, const float* __restrict__ disp,
                                       const float* __restrict__ acc, PixelSet px, int W, int64_t n,
                                       float* __restrict__ out_rgb, float* __restrict__ out_disp,
                                       float* __restrict__ out_acc) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t p = px.pixel(i, W);
    const float a = acc[i];
    for (int c = 0; c < 3; ++c) out_rgb[3 * p + c] = rgb[3 * i + c] + (1.0f - a) * out_rgb[3 * p + c];
    const float d = disp[i];
    out_disp[p] = (d != d) ? 0.0f : d;  // disps[isnan] = 0 (run_nerf.py:140-141)
    if (out_acc) out_acc[p] = a;
}

// one full torch-order feature vector (encode_inputs + embedders, core/raycasters.py:476-555 and
// cutoff_embedder.py:111-174) of point p and ray direction d under the joint transforms S (NJ x 16)
__device__ void encode_row(const ModelDev& M, const float* __restrict__ skts, float px, float py, float pz, float dx,
                           float dy, float dz, float* __restrict__ f) {
    const int nj = M.nj, nv = 1 + 2 * M.mr;
    const int cx = nj * nv + 3 * nj;
    for (int j = 0; j < nj; ++j) {
        float S[12];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) S[4 * r + c] = skts[j * 16 + 4 * r + c];
        float qx, qy, qz;
        joint_local(S, px, py, pz, qx, qy, qz);
        const float dist = norm3(qx, qy, qz);
        const float dn = fmaxf(dist, 1e-12f);
        const float w = M.use_cutoff ? cutoff_w(M.tau, dist, M.cutoff[j]) : 1.0f;
        float u, uf;
        kp_inputs(M.cut_to, M.shift_in, dist, M.cutoff[j], u, uf);
        f[j] = (M.use_cutoff && M.cutoff_inputs) ? u * w : u;
        for (int fi = 0; fi < M.mr; ++fi) {
            float s, c;
            sincosf(uf * (float)(1 << fi), &s, &c);
            f[(1 + 2 * fi) * nj + j] = s * w;
            f[(2 + 2 * fi) * nj + j] = c * w;
        }
        // bone directions, times w_b under --cutoff_bones (bone CutoffEmbedder, multires_bones 0)
        const float wb = M.bone_cut ? cutoff_w(M.tau_b, dist, M.cutoff_b[j]) : 1.0f;
        f[nj * nv + 3 * j + 0] = M.bone_cut ? (qx / dn) * wb : qx / dn;
        f[nj * nv + 3 * j + 1] = M.bone_cut ? (qy / dn) * wb : qy / dn;
        f[nj * nv + 3 * j + 2] = M.bone_cut ? (qz / dn) * wb : qz / dn;
        float ex, ey, ez;
        joint_rot(S, dx, dy, dz, ex, ey, ez);
        const float en = M.view_raw ? 1.0f : fmaxf(norm3(ex, ey, ez), 1e-12f);  // (world: R_j d itself)
        const float e[3] = {ex / en, ey / en, ez / en};
        const float wv = M.cutoff_viewdir ? cutoff_w(M.tau_v, dist, M.cutoff_v[j]) : 1.0f;
        for (int c = 0; c < 3; ++c) {
            f[cx + 3 * j + c] = (M.cutoff_viewdir && M.cutoff_inputs) ? e[c] * wv : e[c];
            for (int fi = 0; fi < M.mrv; ++fi) {
                float s, co;
                sincosf(e[c] * (float)(1 << fi), &s, &co);
                f[cx + (1 + 2 * fi) * 3 * nj + 3 * j + c] = s * wv;
                f[cx + (2 + 2 * fi) * 3 * nj + 3 * j + c] = co * wv;
            }
        }
    }
}

// full torch-order feature vectors, one thread per point
__global__ void encode_points_kernel(ModelDev M, const float* __restrict__ skts, const float* __restrict__ pts,
                                     const float* __restrict__ dirs, int64_t n, float* __restrict__ feat) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int F = M.nj * (1 + 2 * M.mr) + 3 * M.nj + 3 * M.nj * (1 + 2 * M.mrv);
    encode_row(M, skts, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2],
               feat + i * F);
}

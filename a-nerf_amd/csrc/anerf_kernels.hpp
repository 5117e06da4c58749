// anerf_kernels.hpp — the templated __global__ kernels: fused render kernel, density-only kernel, radiance-at-points kernel.
// Included, in order, by anerf_render.hip and by anerf_render_f16.hip (the fp16 instances); the small kernels are anerf_kernels_small.hpp.
#pragma once

// ======================================================================= fused render kernel
// The rays [ray0, ray0 + R) of one workgroup.  FUSED (single_net models, render_fused_kernel): both passes end to
// end, composited and importance-sampled here.  Otherwise (render_kernel) the launch's one pass up to the raws, which
// go to the workspace (A.raw_ws) for render_coarse_stage_kernel / render_fine_stage_kernel (anerf_kernels_small.hpp):
// those stages are sequential double-precision chains on one lane, which this kernel (one wave per SIMD) cannot hide.
template <int W, int MR, int PREC, bool FUSED>
__device__ __forceinline__ void render_item(const ModelDev& M, const RenderArgs& A, const LdsPlan& P,
                                            float* __restrict__ lds, int64_t ray0) {
    constexpr int WH = W / 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = A.R, S = A.S, I = A.I, T = S + I;
    const int nr = (int)min((int64_t)R, A.n - ray0);

    // ---- rays, poses, skeleton transforms into LDS
    for (int r = tid; r < nr; r += blockDim.x) {
        const int64_t i = ray0 + r;
        const float* src = A.rb + i * A.stride;
        float* d = lds + P.ray + 16 * r;
        for (int c = 0; c < 6; ++c) d[c] = src[c];
        d[6] = A.cams ? A.cams[i] : -1.0f;
        d[7] = A.near[i];
        d[8] = A.far[i];
        d[9] = norm3(src[3], src[4], src[5]);
        d[10] = __int_as_float(A.ray_pose ? A.ray_pose[i] : 0);
    }
    __syncthreads();
    for (int idx = tid; idx < nr * M.nj * 12; idx += blockDim.x) {
        const int r = idx / (M.nj * 12), e = idx % (M.nj * 12);
        const int j = e / 12, c = e % 12;
        const int pose = __float_as_int(lds[P.ray + 16 * r + 10]);
        // (an out-of-range pose index renders NaN and is never dereferenced)
        lds[P.sk + P.sk_stride * r + e] = (pose >= 0 && pose < A.n_poses) ? A.skts[((int64_t)pose * M.nj + j) * 16 + c]
                                                                           : __int_as_float(0x7fc00000);
    }
    stage_cut(M, lds + P.cut, tid);
    // coarse samples (sample_from_lineseg, ray_utils.py:218-224)
    if (FUSED || A.pass0 == 0)
        for (int idx = tid; idx < nr * S; idx += blockDim.x) {
            const int r = idx / S, s = idx % S;
            const float t = torch_linspace01(s, S);
            const float nearv = lds[P.ray + 16 * r + 7], farv = lds[P.ray + 16 * r + 8];
            lds[P.zc + P.z_stride * r + s] = lineseg_z(nearv, farv, t, A.lindisp != 0);
        }
    if (!FUSED && A.pass0 == 1) {  // fine-only launch: the sorted fine z the coarse stage kernel left (P.zf == P.zc)
        // (16 B per lane: the item's nr x T floats are one contiguous run, rows 16-B aligned)
        if (T % 4 == 0 && (reinterpret_cast<uintptr_t>(A.zf_ws) & 15) == 0) {
            const f32x4* src = reinterpret_cast<const f32x4*>(A.zf_ws + ray0 * T);
            for (int idx = tid; idx < nr * T / 4; idx += blockDim.x) {
                const int r = (4 * idx) / T, s = (4 * idx) % T;
                *reinterpret_cast<f32x4*>(lds + P.zf + P.z_stride * r + s) = __builtin_nontemporal_load(src + idx);
            }
        } else {
            for (int idx = tid; idx < nr * T; idx += blockDim.x) {
                const int r = idx / T, s = idx % T;
                lds[P.zf + P.z_stride * r + s] = __builtin_nontemporal_load(A.zf_ws + (ray0 + r) * T + s);
            }
        }
    }
    __syncthreads();

    Stamps st;
    STAMP_INIT(st);
    STAMP(st, 0);
    const int n_pass = I > 0 ? 2 : 1;
    for (int pass = A.pass0; pass < min(A.pass1, n_pass); ++pass) {
        const NetDev& net = M.net[pass];
        const int n = pass == 0 ? S : T;
        const int zoff = pass == 0 ? P.zc : P.zf;
        // single_net fine pass (raycasters.py:462-468): the same network on the I new samples only
        // (z_is, left by importance() in the ray's scratch at 6 z_stride), raws after the coarse ones
        // (cat([raw, raw_is]) order), merged by sorted_idx below; biases and G are still in LDS
        const bool only_new = FUSED && pass == 1 && M.single_net;
        if (!only_new) {
            stage_bias<W>(M, net, lds + P.bias, tid);  // (synced below)
            if (M.mrv == 0) compute_view_factor<WH, 0>(M, net, lds, P, nr, tid, st);
            else compute_view_factor<WH, 4>(M, net, lds, P, nr, tid, st);
        }
        STAMP(st, 1);
        // ---- MLP over 32-sample blocks, four at a time (one per wave)
        const int nm = only_new ? I : n;
        const int nb = (nm + 31) / 32, nbt = nr * nb;
        auto block_z = [&](int r) {
            return only_new ? lds + P.scr + P.scr_stride * r + 6 * P.z_stride : lds + zoff + P.z_stride * r;
        };
        int* const bcnt = reinterpret_cast<int*>(lds + P.bord);
        int* const bord = bcnt + P.bord_n;
        if constexpr (lockstep_mode<PREC>()) {
            // bf16x6: the four waves meet at a workgroup barrier before every hidden layer (L1 sharing of
            // the weight stream), where a wave whose block has fewer live joints waits for the others
            // (5.8 % of the wave-cycles, profiles/r04c_stamps_bf16x6.txt).  The blocks of the workgroup
            // run in ascending order of their live-joint counts, so the four blocks of an iteration have
            // about equal windowed work.  (Outputs are unchanged: a block's arithmetic does not depend on
            // the wave that runs it.)  Ties go by depth index, then ray: the same depth range of the item's
            // adjacent pixels is empty together, so an iteration's four blocks tend to be dead together
            // (mlp_block's skip_dead), and only then does the iteration end sooner: a wave that skips
            // alone waits at the next block's first barrier.
            for (int b = wave; b < nbt; b += 4) {
                const int r = b / nb;
                const int c = block_live_count(M, lds + P.ray + 16 * r, lds + P.sk + P.sk_stride * r, lds + P.cut,
                                               block_z(r), nm, (b % nb) * 32, lane);
                if (lane == 0) bcnt[b] = c;
            }
            __syncthreads();
            for (int i = tid; i < nbt; i += blockDim.x) {
                const int ci = bcnt[i], ki = (i % nb) * nr + i / nb;
                int rank = 0;
                for (int j = 0; j < nbt; ++j) {
                    const int cj = bcnt[j], kj = (j % nb) * nr + j / nb;
                    rank += (cj < ci) | ((cj == ci) & (kj < ki));
                }
                bord[rank] = i;
            }
            __syncthreads();
        }
        // (the same trip count on every wave: bf16x6's mlp_trunk has a workgroup barrier per hidden
        // layer; a wave past the last block redoes that block without storing or counting it)
        for (int it = 0; it < (nbt + 3) / 4; ++it) {
            const bool own = it * 4 + wave < nbt;
            if constexpr (!lockstep_mode<PREC>())  // (no workgroup barrier inside: a wave without a block is done)
                if (!own) break;
            const int bi = own ? it * 4 + wave : nbt - 1;
            const int b = lockstep_mode<PREC>() ? bord[bi] : bi;
            const int r = b / nb, s0 = (b % nb) * 32;
            const float* zr = block_z(r);
            float* rawr = FUSED ? lds + P.raw + P.raw_stride * r + (only_new ? 4 * S : 0)
                                : A.raw_ws + (ray0 + r) * n * 4;
            mlp_block<W, MR, PREC, !FUSED>(M, net, lds + P.ray + 16 * r, lds + P.sk + P.sk_stride * r, lds + P.cut,
                             zr, nm, s0, lds + P.g + P.g_stride * r, rawr, lane, own ? A.mfma_count : nullptr,
                             lds + P.bias, (P.uf >= 0 && M.skip + 1 < M.D) ? lds + P.uf + wave * P.uf_stride : nullptr,
                             lds + P.wv + wave * P.wv_stride, st, own, A.skip_dead != 0);
        }
        STAMP(st, 2 + 2 * pass);
        if constexpr (!FUSED) break;  // (one pass per launch; the kernel's item loop has the barrier before the next item)
        __syncthreads();
        STAMP(st, 6);
        // ---- composite (+ importance sampling after the coarse pass); one wave per ray
        for (int r0 = 0; r0 < R; r0 += 4) {
            // (the wave index as a scalar here: the ray index and the output pointers become wave-uniform SGPR
            // values instead of 64-bit per-lane pointers the allocator kept live, spilled, across the MLP)
            const int r = r0 + __builtin_amdgcn_readfirstlane(wave);
            const bool active = r < nr;
            const int64_t i = ray0 + r;
            const float* ray = lds + P.ray + 16 * min(r, R - 1);
            const float* z = lds + zoff + P.z_stride * min(r, R - 1);
            float* raw = lds + P.raw + P.raw_stride * min(r, R - 1);
            float* scr = lds + P.scr + P.scr_stride * min(r, R - 1);
            if (only_new) {  // raw = cat([raw, raw_is])[sorted_idx] (_merge_encodings on 'raw', :466-468)
                const int* src = reinterpret_cast<const int*>(scr + 7 * P.z_stride);
                if (active)
                    for (int k = lane; k < T; k += 64)
                        *reinterpret_cast<f32x4*>(scr + 4 * k) = *reinterpret_cast<const f32x4*>(raw + 4 * src[k]);
                wave_sync();
                if (active)
                    for (int k = lane; k < T; k += 64)
                        *reinterpret_cast<f32x4*>(raw + 4 * k) = *reinterpret_cast<const f32x4*>(scr + 4 * k);
                wave_sync();
            }
            const bool final_pass = pass == n_pass - 1;
            float* o_rgb = final_pass ? A.rgb : A.rgb0;
            float* o_disp = final_pass ? A.disp : A.disp0;
            float* o_acc = final_pass ? A.acc : A.acc0;
            float* o_alpha = final_pass ? A.alpha : A.alpha0;
            float* pal = (active && o_alpha) ? o_alpha + i * n : nullptr;
            if (active) {
                float* dz = pass == 0 ? A.dbg_z0 : A.dbg_z1;
                float* draw = pass == 0 ? A.dbg_raw0 : A.dbg_raw1;
                for (int s = lane; s < n; s += 64) {
                    if (dz) dz[i * n + s] = z[s];
                    if (draw)
                        for (int c = 0; c < 4; ++c) draw[(i * n + s) * 4 + c] = raw[4 * s + c];
                }
            }
            float* res = scr + 7 * P.z_stride;
            composite(M, ray, z, raw, n, scr, P.z_stride, active, lane, pal, res);
            if (active && lane < 5) {
                const float v = res[lane];
                if (lane < 3) {
                    if (o_rgb) o_rgb[3 * i + lane] = v;
                } else if (lane == 3) {
                    if (o_disp) o_disp[i] = v;
                } else if (o_acc) {
                    o_acc[i] = v;
                }
            }
            if (pass == 0 && I > 0) {
                if (active && A.dbg_w0)
                    for (int s = lane; s < S; s += 64) A.dbg_w0[i * S + s] = scr[s];
                importance(z, scr, S, I, lds + P.zf + P.z_stride * min(r, R - 1), scr + P.z_stride, active, lane,
                           nullptr, M.single_net != 0, M.single_net ? reinterpret_cast<int*>(scr + 7 * P.z_stride) : nullptr,
                           M.single_net ? scr + 6 * P.z_stride : nullptr);
            }
        }
        __syncthreads();
        STAMP(st, 3 + 2 * pass);
    }
    STAMP_FLUSH(st, A.stamps);
}

// One launch of the render pass(es): as many workgroups as are resident at
// once (the host sizes the grid by occupancy), each taking R-ray items from eight queues, queue g = the
// g-th contiguous band of the ray list, starting with its own (blockIdx & 7: workgroups b and b + 8
// share an XCD under the round-robin dispatch — a locality choice only, correctness does not depend on
// it) and stealing from the others when it is empty, so each XCD's L2 sees the live joints of one band
// of the frame while the stealing evens out the bands' different costs (round 3's static XCD bands
// lost 5 % to exactly that imbalance); +3.6 % fp16x4, outputs bit-identical (an item's arithmetic does
// not depend on the workgroup that runs it; one workgroup per item: removed, code in 914abec).
template <int W, int MR, int PREC, bool FUSED>
__device__ __forceinline__ void render_items(const ModelDev& M, const RenderArgs& A, const LdsPlan& P) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int64_t items = (A.n + A.R - 1) / A.R;
    int* const slot = reinterpret_cast<int*>(lds + P.bord) + 2 * P.bord_n;
    const int g0 = blockIdx.x & 7;
    for (;;) {
        if (threadIdx.x == 0) {
            int64_t item = -1;
            for (int k = 0; k < 8 && item < 0; ++k) {
                const int g = (g0 + k) & 7;
                const int64_t b0 = items * g / 8, b1 = items * (g + 1) / 8;
                if (b1 <= b0) continue;
                const unsigned t = atomicAdd(A.queue + g, 1u);
                if ((int64_t)t < b1 - b0) item = b0 + t;
            }
            slot[0] = (int)item;
        }
        __syncthreads();
        const int item = slot[0];
        if (item < 0) break;
        render_item<W, MR, PREC, FUSED>(M, A, P, lds, (int64_t)item * A.R);
        __syncthreads();
    }
}

// One pass (A.pass0) up to the raws: every model with two networks, and every model without importance sampling.
template <int W, int MR, int PREC>
__global__ __launch_bounds__(256, 1) void render_kernel(ModelDev M, RenderArgs A, LdsPlan P) {
    render_items<W, MR, PREC, false>(M, A, P);
}

// single_net models: both passes, the composite and the importance sampling in one launch (the fine pass merges the
// coarse raws in LDS by sorted_idx, so there is no second launch to cut at).
template <int W, int MR, int PREC>
__global__ __launch_bounds__(256, 1) void render_fused_kernel(ModelDev M, RenderArgs A, LdsPlan P) {
    render_items<W, MR, PREC, true>(M, A, P);
}

// ======================================================================= density-only queries
// RayCaster.render_pts_density / render_mesh_density (core/raycasters.py:579-648): the trunk of
// one network and alpha_linear at arbitrary points (or at the (res+1)^3 mesh grid, generated here:
// point (a, b, c) = (t[b], t[a], t[c]) + kp0, the 'xy' meshgrid order of the reference).
struct DensityArgs {
    const float* pts;  // N x 3, or NULL for the grid
    const float* t;    // grid axis, res1 floats
    const float* kp0;  // 3
    int64_t res1;
    int64_t n;
    const float* skts;  // NJ x 16, one pose
    int net;
    float* out;  // N raw densities
};

__host__ __device__ inline LdsPlan make_density_plan(int nj, int W, int D, int njh2, bool bone_cut) {
    LdsPlan p;
    std::memset(&p, 0, sizeof(p));
    int o = 0;
    p.sk = o; o += 12 * nj;
    p.cut = o; o += (bone_cut ? 4 : 3) * nj;
    o = (o + 3) & ~3;
    p.bias = o; o += (D + 2) * W;
    p.uf_stride = 64 * 3 * njh2;
    p.uf = o; o += 4 * p.uf_stride;
    p.total = (o + 3) & ~3;
    return p;
}

template <int W, int MR, int PREC>
__global__ __launch_bounds__(256, 1) void density_kernel(ModelDev M, DensityArgs A, LdsPlan P) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int RB = W / 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5;
    const NetDev& net = M.net[A.net];
    for (int idx = tid; idx < M.nj * 12; idx += blockDim.x) lds[P.sk + idx] = A.skts[(idx / 12) * 16 + idx % 12];
    stage_cut(M, lds + P.cut, tid);
    stage_bias<W>(M, net, lds + P.bias, tid);
    __syncthreads();
    Stamps st;
    float* uf = (M.skip + 1 < M.D) ? lds + P.uf + wave * P.uf_stride : nullptr;
    const float* wa = lds + P.bias + (M.D + 1) * W + hh * (W / 2);
    const int64_t nb = (A.n + 31) / 32;
    // (the same trip count on every wave: bf16x6's mlp_trunk has a workgroup barrier per hidden layer;
    // a wave past the last block redoes it without storing)
    for (int64_t base = (int64_t)blockIdx.x * 4; base < nb; base += (int64_t)gridDim.x * 4) {
        const bool own = base + wave < nb;
        if constexpr (!lockstep_mode<PREC>())
            if (!own) break;
        const int64_t b = own ? base + wave : nb - 1;
        const int64_t s_out = b * 32 + (lane & 31);
        const int64_t s = s_out < A.n ? s_out : A.n - 1;
        float px, py, pz;
        if (A.pts) {
            px = A.pts[3 * s], py = A.pts[3 * s + 1], pz = A.pts[3 * s + 2];
        } else {
            const int64_t a = s / (A.res1 * A.res1), r = s % (A.res1 * A.res1);
            px = A.t[r / A.res1] + A.kp0[0];
            py = A.t[a] + A.kp0[1];
            pz = A.t[r % A.res1] + A.kp0[2];
        }
        f32x16 acc[RB], h[RB];
        JointMask mask;
        Ring ring;
        int es = 0;
        mlp_trunk<W, MR, false, PREC, true>(M, net, lds + P.sk, lds + P.cut, px, py, pz, lane, lds + P.bias, uf, nullptr, acc, h, ring,
                         mask, nullptr, st, es);
        // alpha_linear on relu(h_last), in the k-step order of the render path's fused alpha head
        float sig = 0.0f;
#pragma unroll
        for (int q = 0; q < W / 2; ++q) sig = fmaf(wa[q], relu_act(acc[q >> 4][q & 15]), sig);
        if constexpr (PREC >= 3) sig *= pow2f(-es);  // (fp16x3 / fp16x4: the last layer's units)
        sig += __shfl_xor(sig, 32);
        sig += net.balpha;
        if (own && hh == 0 && s_out < A.n) A.out[s_out] = sig;
    }
}

// ======================================================================= radiance at points
// anerf_radiance_points (RayCaster.render_pts_radiance): a whole network at arbitrary points, every point with
// its own ray direction -- raw (rgb, sigma) as mlp_block leaves it.  The density kernel's block loop; after the
// trunk the fused feature + view layer with the alpha head folded in, exactly as mlp_block.  The render kernel
// factorises the view layer's direction part per ray (compute_view_factor -> G -> view_dir_part), which needs
// the 32 samples of a block to share a ray; here the lanes form their own windowed view features and feed them
// as B operands of f32 k-steps against the direction columns of the view weights:
//
//   k-step (p, t), p < NJH2, t < 3 NK:   lane half h holds joint j = p + h NJH2 (the u part's pairing, so w'_j
//       is the value the u part stored per lane), term t = 3 k + c of the trig table (k = 0: e_c, 1 + 2f: sin,
//       2 + 2f: cos of e_c 2^f; e = R_j d, normalised unless view_raw);
//       A = wvdir[j][32 rb + (l & 31)][t]   (the row's TP floats are contiguous: 16-B loads)
//       B = T_t(e_j) * (w'_j where the term is windowed, else 1) * 2^es   (0 for a padding joint)
//   last k-step:  A = bias / framecode column (LDS, once per workgroup; half 1: 0), B = 2^es (half 1: 0).
//
// fp32 in every precision mode, as view_dir_part.  A pair p whose windows are exactly 0 at every point of the
// block adds exact zeros and is skipped (wave-uniform) when every term is windowed.
struct RadianceArgs {
    const float* pts;    // N x 3
    const float* dirs;   // N x 3, or 1 x 3 with dir_stride 0
    int64_t dir_stride;  // floats between two points' directions (3 or 0)
    int64_t n;
    const float* skts;   // NJ x 16, one pose
    float cam;           // framecode index (< 0: the mean code)
    int net;
    float* out;          // N x 4
};

__host__ __device__ inline LdsPlan make_radiance_plan(int nj, int W, int D, int njh2, bool bone_cut) {
    LdsPlan p = make_density_plan(nj, W, D, njh2, bone_cut);
    int o = p.total;
    p.wv_stride = 64 * (njh2 + 1);  // per wave: the block's view windows w'_j (+ a discard row), as make_plan
    p.wv = o; o += 4 * p.wv_stride;
    p.g = o; o += W / 2;            // the bias / framecode column of the view layer
    p.total = (o + 3) & ~3;
    return p;
}

template <int RBV, int MRV>
__device__ __forceinline__ void view_dir_points(f32x16 (&av)[RBV], const ModelDev& M, const NetDev& net,
                                                const float* __restrict__ sk, const float* __restrict__ wvp,
                                                const float* __restrict__ vb, float dx, float dy, float dz, int lane,
                                                float bs) {
    constexpr int WH = RBV * 32, NK = 1 + 2 * MRV, KC = 3 * NK, TP = (KC + 3) & ~3;
    const int hh = lane >> 5, sl = lane & 31;
    const int njh2 = M.njh2, nj = M.nj;
    const int kfw = M.cutoff_inputs ? 0 : 1;            // first k term multiplied by w' (compute_view_factor)
    const bool cull = M.cutoff_viewdir && kfw == 0;      // every term is windowed
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(net.wvdir);
    for (int p = 0; p < njh2; ++p) {
        const float w = wvp[p * 64 + lane];  // (0 for a padding joint or without cutoff_viewdir, u_joint)
        if (cull && __ballot(w != 0.0f) == 0) continue;  // (a NaN window is live)
        const int j = p + hh * njh2;
        const bool valid = j < nj;
        const int jc = valid ? j : 0;
        float e[3];
        joint_rot(sk + 12 * jc, dx, dy, dz, e[0], e[1], e[2]);
        const float en = M.view_raw ? 1.0f : fmaxf(norm3(e[0], e[1], e[2]), 1e-12f);  // (world: R_j d itself)
        float feat[TP];
        const float s0 = mask_f((M.cutoff_viewdir && kfw == 0) ? w * bs : bs, valid);
        const float s1 = mask_f(M.cutoff_viewdir ? w * bs : bs, valid);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float ec = e[c] / en;
            feat[c] = ec * s0;
#pragma unroll
            for (int f = 0; f < MRV; ++f) {
                float sn, cs;
                sincos_rr(ec * (float)(1 << f), sn, cs);
                // (frequencies past the model's: zero weights in the layout's padding, zero features too)
                feat[(1 + 2 * f) * 3 + c] = f < M.mrv ? sn * s1 : 0.0f;
                feat[(2 + 2 * f) * 3 + c] = f < M.mrv ? cs * s1 : 0.0f;
            }
        }
#pragma unroll
        for (int rb = 0; rb < RBV; ++rb) {
            float wa[TP];
#pragma unroll
            for (int q = 0; q < TP / 4; ++q) {
                const f32x4 x = bload4(rs, (jc * WH + 32 * rb + sl) * TP * 4 + q * 16, 0);
                wa[4 * q] = x[0], wa[4 * q + 1] = x[1], wa[4 * q + 2] = x[2], wa[4 * q + 3] = x[3];
            }
#pragma unroll
            for (int t = 0; t < KC; ++t) av[rb] = mfma_f32_32x32x2(wa[t], feat[t], av[rb]);
        }
    }
#pragma unroll
    for (int rb = 0; rb < RBV; ++rb)
        av[rb] = mfma_f32_32x32x2(hh ? 0.0f : vb[32 * rb + sl], hh ? 0.0f : bs, av[rb]);
}

template <int W, int MR, int PREC>
__global__ __launch_bounds__(256, 1) void radiance_kernel(ModelDev M, RadianceArgs A, LdsPlan P) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int RB = W / 32, RBV = (W / 2) / 32, WH = W / 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5;
    const NetDev& net = M.net[A.net];
    for (int idx = tid; idx < M.nj * 12; idx += blockDim.x) lds[P.sk + idx] = A.skts[(idx / 12) * 16 + idx % 12];
    stage_cut(M, lds + P.cut, tid);
    stage_bias<W>(M, net, lds + P.bias, tid);
    if (tid < WH) {  // bview + Wv_code code, in compute_view_factor's order
        float b = net.bview[tid];
        if (M.cfc) {
            const int64_t row = A.cam < 0.0f ? (int64_t)M.n_codes : (int64_t)A.cam;
            for (int m = 0; m < M.cfc; ++m) b += net.wvcode[m * WH + tid] * net.codes[row * M.cfc + m];
        }
        lds[P.g + tid] = b;
    }
    __syncthreads();
    Stamps st;
    float* uf = (M.skip + 1 < M.D) ? lds + P.uf + wave * P.uf_stride : nullptr;
    float* wvp = lds + P.wv + wave * P.wv_stride;
    const int64_t nb = (A.n + 31) / 32;
    // (the same trip count on every wave, as density_kernel: bf16x6's mlp_trunk has a workgroup barrier per layer)
    for (int64_t base = (int64_t)blockIdx.x * 4; base < nb; base += (int64_t)gridDim.x * 4) {
        const bool own = base + wave < nb;
        if constexpr (!lockstep_mode<PREC>())
            if (!own) break;
        const int64_t b = own ? base + wave : nb - 1;
        const int64_t s_out = b * 32 + (lane & 31);
        const int64_t s = s_out < A.n ? s_out : A.n - 1;  // (the ragged block's lanes redo point n - 1)
        const float px = A.pts[3 * s], py = A.pts[3 * s + 1], pz = A.pts[3 * s + 2];
        const float* dp = A.dirs + s * A.dir_stride;
        const float dx = dp[0], dy = dp[1], dz = dp[2];
        f32x16 acc[RB], h[RB];
        JointMask mask;
        Ring ring;
        int es = 0;
        const bool pre = mlp_trunk<W, MR, true, PREC>(M, net, lds + P.sk, lds + P.cut, px, py, pz, lane, lds + P.bias, uf,
                                                      wvp, acc, h, ring, mask,
                                                      PREC >= 3 ? net.wviewh : (PREC == 2 ? net.wview6 : net.wview), st,
                                                      es);
        float sig = 0.0f;
        f32x16 av[RBV];
        if constexpr (PREC >= 3) {
            const int es_h = es;  // the alpha head sums the last hidden layer's activations, in its units
            mlp_layer_h3<RBV, RB, false, true, PREC == 4 ? 4 : 3>(av, acc, h, nullptr, net.wviewh, lane, ring, pre, nullptr,
                                                                  lds + P.bias + (M.D + 1) * W, sig, es, net.ew_view,
                                                                  M.h3_top);
            sig *= pow2f(-es_h);
        } else if constexpr (PREC == 2)
            mlp_layer_x6<RBV, RB, false, true>(av, acc, h, nullptr, net.wview6, lane, ring, pre, nullptr,
                                               lds + P.bias + (M.D + 1) * W, sig);
        else
            mlp_layer<RBV, RB, true, false, true>(av, acc, h, nullptr, net.wview, lane, ring, nullptr,
                                                  lds + P.bias + (M.D + 1) * W, sig);
        sig += __shfl_xor(sig, 32);
        sig += net.balpha;
        const float bs = PREC >= 3 ? pow2f(es) : 1.0f;  // (the view layer's units: the B operands carry them)
        if (M.mrv == 0) view_dir_points<RBV, 0>(av, M, net, lds + P.sk, wvp, lds + P.g, dx, dy, dz, lane, bs);
        else view_dir_points<RBV, 4>(av, M, net, lds + P.sk, wvp, lds + P.g, dx, dy, dz, lane, bs);
        float rgb[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* wr = net.wrgb + (c * 2 + hh) * RBV * 16;
            float a = 0.0f;
#pragma unroll
            for (int rb = 0; rb < RBV; ++rb)
#pragma unroll
                for (int i = 0; i < 16; ++i) a += wr[rb * 16 + i] * relu_act(av[rb][i]);
            a += __shfl_xor(a, 32);
            if constexpr (PREC >= 3) a *= pow2f(-es);  // (the view layer's units)
            rgb[c] = a + net.brgb[c];
        }
        if (own && hh == 0 && s_out < A.n) {
            float* o = A.out + 4 * s_out;
            o[0] = rgb[0];
            o[1] = rgb[1];
            o[2] = rgb[2];
            o[3] = sig;
        }
    }
}

// ======================================================================= the fp16 instances' unit
// The fp16 instances (PREC 3 and 4) of the three MLP kernels are compiled in anerf_render_f16.hip, the one unit built
// with MFMA results in VGPRs (build.py RENDER_F16_FLAGS: their scale and relu read the accumulators on the VALU, which
// cannot read AGPRs); anerf_render.hip declares them extern and launches them.  KW: `extern` or nothing.
#define ANERF_F16_KERNEL(KW, K, ARGS, WW, MM)                              \
    KW template __global__ void K<WW, MM, 3>(ModelDev, ARGS, LdsPlan);    \
    KW template __global__ void K<WW, MM, 4>(ModelDev, ARGS, LdsPlan);
#ifdef ANERF_AB_FAST  // (tools/build_ab.sh: the config-3 shape only, as the launch tables of anerf_render.hip)
#define ANERF_F16_SHAPES(KW, K, ARGS) ANERF_F16_KERNEL(KW, K, ARGS, 256, 7)
#else
#define ANERF_F16_SHAPES(KW, K, ARGS)                                                                     \
    ANERF_F16_KERNEL(KW, K, ARGS, 256, 7) ANERF_F16_KERNEL(KW, K, ARGS, 128, 7) ANERF_F16_KERNEL(KW, K, ARGS, 64, 7) \
    ANERF_F16_KERNEL(KW, K, ARGS, 256, 10) ANERF_F16_KERNEL(KW, K, ARGS, 128, 10) ANERF_F16_KERNEL(KW, K, ARGS, 64, 10)
#endif
#define ANERF_F16_INSTANCES(KW)                       \
    ANERF_F16_SHAPES(KW, render_kernel, RenderArgs)   \
    ANERF_F16_SHAPES(KW, render_fused_kernel, RenderArgs) \
    ANERF_F16_SHAPES(KW, density_kernel, DensityArgs) \
    ANERF_F16_SHAPES(KW, radiance_kernel, RadianceArgs)

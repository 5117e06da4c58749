/*
 * anerf.h — C ABI of the MI355X-native A-NeRF render path (libanerf_hip.so).
 *
 * Plain pointers and sizes only: every float/int pointer passed to a render or stage entry is
 * a DEVICE pointer (HBM) on the model's device; model creation takes HOST pointers to the
 * reference's weights in their torch layout.  Every entry returns 0 on success or a negative
 * ANERF_E* code; anerf_last_error() returns a thread-local message.  Launch entries never
 * allocate, never synchronise and are safe to capture in a hipGraph; their scratch is the
 * caller's workspace (size from anerf_workspace_size).
 *
 * Reference interfaces replaced (paths relative to danielajisafe/A-NeRF):
 *   anerf_model_create      create_raycaster + RayCaster.load_state_dict      core/raycasters.py:17-184, 768-788
 *   anerf_render_rays       RayCaster.render_rays (eval, perturb=0, no noise)   core/raycasters.py:361-474
 *                           incl. get_near_far_in_cylinder + chunk NaN fill     core/utils/ray_utils.py:292-344
 *                           batchify_rays chunking (NaN-fill granularity)       core/trainer.py:64-79
 *   anerf_gen_rays          get_rays gathered at kp_to_valid_rays' pixel list  core/utils/ray_utils.py:6-28, 127-132
 *   anerf_encode_points     encode_inputs + embedders (stage / debug)          core/raycasters.py:476-555
 *   anerf_near_far          get_near_far_in_cylinder (stage)                   core/utils/ray_utils.py:292-344
 *   anerf_compose           render_path's image composition + NaN disp -> 0    run_nerf.py:100-141
 *   anerf_gen_rays_box,     the same over kp_to_valid_rays' box, the pixel     core/utils/ray_utils.py:127-132
 *   anerf_compose_box       list generated on the device (no index upload)
 *   anerf_density_points    RayCaster.render_pts_density (fwd_type='density')  core/raycasters.py:597-648
 *   anerf_density_grid      RayCaster.render_mesh_density (fwd_type='mesh')    core/raycasters.py:579-595
 *                           (called by run_render.render_mesh)                 run_render.py:970-986
 *   anerf_isosurface_count, mcubes.marching_cubes of run_render.render_mesh    run_render.py:983-984
 *   anerf_isosurface_emit   (the grid's iso-surface as an indexed mesh, ABI 20)
 *   anerf_isosurface_normals   per-vertex normals of that mesh from the grid's gradient (ABI 21; the reference's
 *                           viewer accumulates face normals on the host)       render_mesh.py:35-53
 *   anerf_mesh_components,  the connected components of that mesh and its stable compaction (ABI 22; the reference
 *   anerf_mesh_compact_*    leaves floaters and cavities to the user: trimesh's split() on the host)
 *   anerf_mesh_adjacency_*, the vertex adjacency of that mesh as a CSR and Laplacian / Taubin smoothing over it (ABI 23;
 *   anerf_mesh_smooth       the reference leaves smoothing to the user: trimesh.smoothing.filter_taubin on the host)
 *   anerf_mesh_vertex_normals   compute_normal of the reference's mesh viewer (face normals summed per vertex) and
 *   anerf_mesh_raster       what its OpenGL pass draws: an orthographic view of the mesh (ABI 24)   render_mesh.py:35-54, 164-182
 *   anerf_mesh_simplify_*   vertex clustering of that mesh on a grid of cells (ABI 25; the reference leaves decimation
 *                           to the user: trimesh with open3d or fast_simplification on the host)
 *   anerf_mesh_raster_persp   that mesh through a perspective camera, cut at the near plane (ABI 26; the reference's
 *                           viewer is orthographic: the mesh cannot be drawn where the field is rendered)
 *   anerf_radiance_points   the whole network (raw rgb, sigma) at points with their own directions (ABI 21)
 *                                                                              core/networks/nerf.py:133-148
 *   anerf_pose_kinematics   PoseOptLayer.calculate_kinematic, get_smpl_l2ws    core/pose_opt.py:372-521,
 *   anerf_pose_kinematics_backward   its autograd (pose optimisation)
 *                                                                              core/utils/skeleton_utils.py:296-376
 *   anerf_kp_boxes          kp_to_valid_rays' cylinder + pixel box             core/utils/ray_utils.py:83-136
 *   anerf_ray_batch         BaseH5Dataset.__getitem__ + ray_collate_fn (the    core/dataset.py:57-105, 259-275,
 *                           training ray sampler) over HBM-resident images     346-364, 796-802
 *   anerf_gather_rows       ray_collate_fn's per-ray pose rows                 core/dataset.py:96-104, 796-802
 * Training stages of render_rays (perturb, raw noise, stochastic importance sampling, gradients):
 *   anerf_train_samples     sample_from_lineseg (perturb > 0)                  core/utils/ray_utils.py:204-251
 *   anerf_train_encode      sample_pts + encode_inputs (+ embedders)           core/raycasters.py:476-555, 650-663
 *   anerf_train_encode_backward   autograd of the same to skts (pose opt.)     core/encoders.py:8-37, 101-193,
 *                                                                              core/cutoff_embedder.py:111-174
 *   anerf_train_composite   NeRF.raw2outputs with raw_noise_std                core/networks/nerf.py:150-205
 *   anerf_train_composite_backward   its autograd
 *   anerf_train_importance  isample_from_lineseg + sample_pdf(det=False) + sort core/utils/ray_utils.py:157-201, 255-289
 *   anerf_train_view_factor (+ _backward)   per-ray view factors of the view-window layout
 *   anerf_train_view_mix (+ _backward)   the view layer's view part in the view-window layout
 *                           (ANERF_ENC_VIEW_WINDOWS; views_linears.0 on the view columns, core/networks/nerf.py:141-148)
 * The training MLP's linears (NeRF.forward / autograd, core/networks/nerf.py:94-148; the reference runs
 * them as torch addmm over cat()-ed inputs, core/raycasters.py:557-577):
 *   anerf_mlp_split_weights a weight (or its transpose) as bf16 hi / lo planes, once per step
 *   anerf_mlp_split_weights_batch   the same for up to 32 weights in one launch
 *   anerf_mlp_gemm          forward (bias, relu) and input-gradient (relu' mask, accumulate) products
 *   anerf_mlp_wgrad         weight + bias gradients
 *   anerf_mlp_backward_hidden  both of a 256 x 256 hidden layer's backward products in one pass (round 6)
 *   anerf_mlp_backward_head    the same for feature_linear with alpha_linear's rank-1 term (round 6, ABI 18)
 *   anerf_mlp_forward_hidden   a 256 x 256 hidden layer's forward, persistent (round 6, ABI 19)
 *   anerf_mlp_forward_layer    the same for any 256-output layer: layer 0, the skip layer, the heads (ABI 19)
 *   anerf_mlp_gemm_persistent  the same kernel as a product of any width (the feature gradient, ABI 19)
 *   anerf_mlp_forward(_pack)  the whole forward in one kernel (opt-in alternative to the GEMMs)
 * The tail of a training step (Trainer.compute_loss / optimize):
 *   anerf_train_loss (+ _backward)   Trainer._compute_nerf_loss, fine and coarse    core/trainer.py:353-380
 *   anerf_pose_loss (+ _backward)    Trainer._compute_kp_loss                        core/trainer.py:382-441
 *   anerf_adam_step         torch.optim.Adam's update over a table of tensors + get_gradnorm   core/trainer.py:191-203
 */
#ifndef ANERF_H
#define ANERF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ANERF_ABI_VERSION 26

enum {
    ANERF_OK = 0,
    ANERF_EINVAL = -1,      /* bad argument / unsupported configuration */
    ANERF_EHIP = -2,        /* HIP runtime error */
    ANERF_EWORKSPACE = -3,  /* workspace too small */
    ANERF_ENOMEM = -4
};

/* arithmetic used for the MLP contractions:
 *   ANERF_PREC_FP32   every contraction on v_mfma_f32_32x32x2_f32 (exact fp32 products);
 *   ANERF_PREC_BF16X3 the dense hidden layers split as x = x_hi + x_lo (bf16, round to nearest even)
 *                     and computed as x_hi w_hi + x_hi w_lo + x_lo w_hi on v_mfma_f32_32x32x16_bf16
 *                     with fp32 accumulation (~16-bit operands, products exact): outputs within
 *                     1e-5 of the fp32 path on the reference fixtures; encoder and view parts fp32;
 *   ANERF_PREC_BF16X6 the dense hidden layers and the fused view layer split three ways: activations
 *                     x = x0 + x1 + x2 exactly (truncation: 8 + 8 + 8 significant bits), weights
 *                     w = w0 + w1 + w2 (bf16 RNE of the running remainder), computed as the six products
 *                     with i + j <= 2 of x_i w_j on v_mfma_f32_32x32x16_bf16, fp32 accumulation: the
 *                     dropped terms are below 2^-23 of each product (fp32 rounds a product to 2^-24),
 *                     so the contraction is fp32-accurate; layer 0's and the skip layer's bone-direction
 *                     parts the same way, and their windowed (per-joint sin/cos) parts too at widths
 *                     128 / 256 (fp32 at width 64); encoder and heads fp32;
 *   ANERF_PREC_FP16X3 the dense hidden layers and the fused view layer in fp16 after exact power-of-two
 *                     scaling (weights per layer, activations per sample, both to a maximum in
 *                     [2^10, 2^11)): x = x0 + x1, w = w0 + w1 (22 significant bits each), computed as
 *                     x0 w0 + x0 w1 + x1 w0 on v_mfma_f32_32x32x16_f16 (exact products, fp32 accumulation,
 *                     the dropped x1 w1 ~2^-22 of |x w|): half of bf16x6's MFMAs, 22-bit instead of
 *                     24-bit operands;
 *                     bone-direction parts and (widths 128 / 256) the windowed parts of layer 0 and the
 *                     skip layer as in bf16x6 (fp32 at width 64); encoder and heads fp32;
 *   ANERF_PREC_FP16X4 fp16x3 plus the fourth product x1 w1: the contraction is then (x - r_x)(w - r_w)
 *                     with the split remainders |r_x| <= 2^-23 |x|, |r_w| <= 2^-23 |w|, within ~2^-22 of
 *                     |x w| per product — the bound of bf16x6's dropped terms (x1 w2 + x2 w1 + x2 w2 and
 *                     the weights' third remainder, ~2^-22.2), so fp32-accurate like bf16x6, with four
 *                     MFMAs per 16 k instead of six and two weight planes (4 B per weight) instead of
 *                     three; everything else as fp16x3. */
enum { ANERF_PREC_FP32 = 0, ANERF_PREC_BF16X3 = 1, ANERF_PREC_BF16X6 = 2, ANERF_PREC_FP16X3 = 3, ANERF_PREC_FP16X4 = 4 };
/* Flags OR-ed into anerf_render_rays' precision argument (and anerf_train_samples' flags):
 *   ANERF_FLAG_LINDISP  sample linearly in inverse depth, z = 1 / (1/near (1 - t) + 1/far t)
 *                       (render_rays(lindisp=True), core/utils/ray_utils.py:223-226)
 *   ANERF_FLAG_NEAR_FAR (anerf_render_rays only) ray_batch columns 6 and 7 already hold every ray's
 *                       near / far AFTER get_near_far_in_cylinder and its chunk NaN fill
 *                       (core/utils/ray_utils.py:292-344), e.g. anerf_near_far's outputs over the
 *                       whole chunks that contain the rays: the kernel uses them as they are (cyls
 *                       and chunk are then not read).  Lets a rank render any sub-range of a chunked
 *                       ray list with the single-GPU NaN fill (ray-balanced sharding). */
enum { ANERF_FLAG_LINDISP = 0x100, ANERF_FLAG_NEAR_FAR = 0x200 };

typedef struct anerf_model anerf_model;

/* Shape of the path: the subset of run_nerf.py flags that shapes the kernel. */
typedef struct {
    int32_t n_joints;        /* NJ (24 SMPL, 65 Mixamo-like) */
    int32_t net_depth;       /* netdepth D */
    int32_t net_width;       /* netwidth W: 64, 128 or 256 */
    int32_t skip;            /* skips=[skip]; layer skip+1 consumes [x, h]; >= D-1 means none */
    int32_t multires;        /* kp positional-encoding frequencies (7) */
    int32_t multires_views;  /* view-direction frequencies: 4 (default) or 0 (surreal_single.txt) */
    int32_t use_cutoff;      /* --use_cutoff */
    int32_t cutoff_inputs;   /* --cutoff_inputs */
    int32_t cutoff_viewdir;  /* --cutoff_viewdir (windows the view features only together with use_cutoff, as the
                                reference's create_raycaster builds the view embedder, core/raycasters.py:31, 68-71) */
    int32_t framecode_ch;    /* 0, or --framecode_size when --opt_framecode */
    int32_t n_framecodes;
    int32_t density_softplus;/* 0: relu, 1: softplus(x - softplus_shift) */
    float softplus_shift;
    float density_scale;     /* B in raw2outputs */
    int32_t has_fine;        /* a separate network_fine exists (N_importance > 0, !single_net) */
    int32_t single_net;      /* --single_net: network_fine IS network_fn (raycasters.py:101-104); the fine
                                pass evaluates only the I new samples and merges raws (:462-468), the
                                importance weights are 0.5 (max(w_l,w_k) + max(w_k,w_u)) + 0.01
                                (ray_utils.py:270-277); requires has_fine == 0 */
    int32_t encoder_flags;   /* ANERF_ENC_* (kp embedder options of the cutoff embedder; 0 = none) */
    int32_t multires_bones;  /* --multires_bones (ABI 15): bone-direction frequencies, 0-10 (0: the bare
                                directions, the default); > 0 is a staged encoder (below) */
} anerf_model_desc;

/* Staged encoders (ABI 15): --multires_bones > 0, ANERF_ENC_KP_RELPOS / _KP_QUERYPTS and ANERF_ENC_VIEW_ANGLE change the
 * MLP's input layout beyond what the fused render kernel streams (its layer-0 parts and the per-ray view
 * factor G assume one distance per joint, bare bone directions and per-ray view directions).  A model with
 * any of them ("staged") is served by the training stages -- anerf_train_samples / _encode (+ _backward) /
 * _composite (+ _backward) / _importance with the MLP on anerf_mlp_gemm -- which the Python RayCaster runs
 * deterministically (perturb 0, no noise) for eval renders; anerf_render_rays, anerf_density_points /
 * _grid and anerf_encode_points reject it (ANERF_EINVAL), and anerf_model_create takes no weights for it
 * (the anerf_net_weights pointers may be NULL).  The feature row of a sample is
 *   [kp part | bone part | view part], with
 *   kp part   reldist: NJ (1 + 2 multires) columns, column f NJ + j (f = 0 the input, 2k + 1 / 2k + 2 the sin /
 *             cos of frequency 2^k);  relpos: 3 NJ (1 + 2 multires), column 3 f NJ + 3 j + c;  querypts:
 *             3 (1 + 2 multires), column 3 f + c;
 *   bone part 3 NJ (1 + 2 multires_bones), column 3 f NJ + 3 j + c;
 *   view part relray / world: 3 NJ (1 + 2 multires_views), column 3 f NJ + 3 j + c;
 *             rayangle: NJ (1 + 2 multires_views), column f NJ + j. */

/* anerf_model_desc.encoder_flags: the kp (distance) CutoffEmbedder's input transforms
 * (core/cutoff_embedder.py:125-134, only with use_cutoff): CUT_TO_DIST (--cut_to_dist) feeds
 * c_j - dist to the encoding (the raw input and the frequencies); CUTOFF_SHIFT (--cutoff_shift)
 * feeds (input * (2 / c_j) - 1) to the frequencies only.  The cutoff window keeps the distance. */
#define ANERF_ENC_CUT_TO_DIST 1
#define ANERF_ENC_CUTOFF_SHIFT 2
/* --cutoff_bones (core/raycasters.py:52-64): the bone embedder is a CutoffEmbedder (dist_inputs, its
 * own tau and cutoff_dist: anerf_embed_params tau_b / cutoff_dist_b); with --multires_bones 0 its
 * output is the bone direction times w_b = 1 - sigmoid(tau_b (dist - c_b)) when use_cutoff and
 * cutoff_inputs (core/cutoff_embedder.py:111-166), the bare direction otherwise.  With --multires_bones 0
 * the flag is ignored (and tau_b / cutoff_dist_b unused) unless desc->use_cutoff and desc->cutoff_inputs are
 * both set; with --multires_bones > 0 (staged) it needs use_cutoff only: the sin / cos features are windowed
 * by w_b either way, the bare directions with cutoff_inputs. */
#define ANERF_ENC_CUTOFF_BONES 4
/* --view_type world (core/raycasters.py:279-280, ABI 14): the view input of joint j is R_j d itself
 * (IdentityExpandEncoder of transform_batch_rays, encoders.py:25-37, 71-79), not the normalised
 * R_j d / |R_j d| of the default relray (VecNormEncoder, encoders.py:172-193).  Rendering, and (round 5)
 * anerf_train_encode / _encode_backward (the identity's gradient in place of the normalisation's). */
#define ANERF_ENC_VIEW_RAW 8
/* --kp_dist_type relpos (core/encoders.py:124-142, raycasters.py:261-262; staged, ABI 15): the kp input of joint
 * j is its local point q_j (3 values) instead of |q_j|; the kp CutoffEmbedder then has dist_inputs (the window
 * of all three from the joint distance, no cut_to_dist / cutoff_shift transform, cutoff_embedder.py:115-121)
 * and the reference's window distance |p - kp_j| is not a function of the poses (raycasters.py:530-533): its
 * gradient to skts is 0, for every windowed embedder of such a model. */
#define ANERF_ENC_KP_RELPOS 16
/* --view_type rayangle (core/encoders.py:195-212, skeleton_utils.py:594-605; staged, ABI 15): the view input
 * of joint j is one angle, acos(clamp(q_j . R_j d / (|q_j| |R_j d|), -1 + 1e-6, 1 - 1e-6)) - pi / 2. */
#define ANERF_ENC_VIEW_ANGLE 32
/* --kp_dist_type querypts (core/raycasters.py:263-265, IdentityEncoder(1, 3); staged, ABI 15): the kp input is the
 * world point p itself (3 values, not per joint); the kp CutoffEmbedder then has cutoff_dim 3 (embed->cutoff_dist
 * holds 3 values, not NJ) and windows each coordinate by itself, w_c = 1 - sigmoid(tau (p_c - c_c))
 * (cutoff_embedder.py:122-144: dists = inputs; --cut_to_dist / --cutoff_shift apply to the encoded values).  No
 * gradient reaches skts through it.  Not with ANERF_ENC_CUTOFF_BONES (the reference's bone CutoffEmbedder then
 * gets cutoff_dim 3 for 3 NJ inputs and fails). */
#define ANERF_ENC_KP_QUERYPTS 64
/* Training layout of the view part (ABI 16; anerf_train_encode / _encode_backward only, the other entry points
 * ignore the flag): the view part of a feature row is the NJ view windows w_j = 1 - sigmoid(tau_v (dist_j - c_v,j))
 * (column cv + j, cv = the view part's first column) instead of the 3 NJ (1 + 2 multires_views) windowed
 * direction features.  Every one of those features is w_j times a function of the ray alone (R_j d), so the
 * view layer's product with them is sum_j w_j G_j(ray) with G_j = Wv_j T_j(R_j d) per ray: the caller forms
 * T, G and that sum (the view direction's gradient to skts included) and the encoder handles the windows
 * (their gradient in _encode_backward's g_feat column cv + j).  Needs cutoff_viewdir, use_cutoff and cutoff_inputs
 * (every direction feature windowed); not with ANERF_ENC_VIEW_ANGLE or a staged encoder. */
#define ANERF_ENC_VIEW_WINDOWS 128

/* HOST pointers to one NeRF's weights, torch nn.Linear layout [out][in] (core/networks/nerf.py:57-88). */
typedef struct {
    const float* pts_w[16];  /* pts_linears[i].weight, i < net_depth */
    const float* pts_b[16];
    const float* alpha_w;    /* alpha_linear  [1][W]   */
    const float* alpha_b;    /* [1] */
    const float* feature_w;  /* feature_linear [W][W] */
    const float* feature_b;
    const float* views_w;    /* views_linears.0 [W/2][W + 3NJ(1+2*multires_views) + framecode_ch] */
    const float* views_b;
    const float* rgb_w;      /* rgb_linear [3][W/2] */
    const float* rgb_b;
    const float* codes;      /* framecodes.codes.weight [n_framecodes][framecode_ch] or NULL */
} anerf_net_weights;

/* HOST pointers to the embedders' state (core/cutoff_embedder.py:91-95). */
typedef struct {
    const float* cutoff_dist;    /* embed_fn.cutoff_dist [NJ]     */
    float tau;                   /* embed_fn.tau                  */
    const float* cutoff_dist_v;  /* embeddirs_fn.cutoff_dist [NJ] */
    float tau_v;                 /* embeddirs_fn.tau              */
    const float* cutoff_dist_b;  /* embedbones_fn.cutoff_dist [NJ] (ANERF_ENC_CUTOFF_BONES), else NULL */
    float tau_b;                 /* embedbones_fn.tau             */
} anerf_embed_params;

/* Optional per-stage outputs of anerf_render_rays (any member may be NULL). */
typedef struct {
    float* near;      /* [N]   after the chunk NaN fill */
    float* far;       /* [N]   */
    float* z_coarse;  /* [N][S] */
    float* raw_coarse;/* [N][S][4] (rgb, sigma) */
    float* weights0;  /* [N][S] */
    float* z_fine;    /* [N][S+I] sorted merged samples */
    float* raw_fine;  /* [N][S+I][4] */
    unsigned long long* mfma_count; /* [2] += MFMA instructions issued, a kernel-side tally of the
                                       work (agrees with PMC SQ_INSTS_MFMA): [0] v_mfma_f32_32x32x2_f32,
                                       [1] the 16-bit MFMAs, v_mfma_f32_32x32x16_bf16 (bf16x3 / bf16x6
                                       modes, and the bf16x6 bone-direction parts of fp16x3) and
                                       v_mfma_f32_32x32x16_f16 (fp16x3), the same FLOPs and cycles each.
                                       The tally is a diagnostic call's (debug != NULL), which runs every
                                       32-sample block in full; a product call (debug == NULL, relu density)
                                       issues fewer MFMAs by the view layer and view-direction part of the
                                       blocks whose 32 densities are all zero, which it leaves out */
} anerf_debug;

int anerf_abi_version(void);
const char* anerf_last_error(void);

/* Pack (on the host) and upload one model to `device`. fine may be NULL when !has_fine. */
int anerf_model_create(const anerf_model_desc* desc, const anerf_net_weights* coarse,
                       const anerf_net_weights* fine, const anerf_embed_params* embed, int device,
                       anerf_model** out);
int anerf_model_destroy(anerf_model* m);
/* Replace the embedders' state of a model without repacking its weights: tau / tau_v / tau_b always,
 * cutoff_dist / cutoff_dist_v / cutoff_dist_b when not NULL (then synchronously, after the device has
 * drained).
 * Launches issued afterwards use the new values: the tau schedule of training
 * (RayCaster.update_embed_fns -> CutoffEmbedder.update_tau, core/raycasters.py:731-748,
 * core/cutoff_embedder.py:176-183).  Not thread-safe against concurrent launches on the model. */
int anerf_model_set_embed(anerf_model* m, const anerf_embed_params* embed);
/* bytes of packed device weights held by the model */
size_t anerf_model_bytes(const anerf_model* m);

/* Scratch bytes anerf_render_rays needs for n_rays rays. */
size_t anerf_workspace_size(const anerf_model* m, int64_t n_rays, int32_t n_samples, int32_t n_importance);

/*
 * Render n_rays rays (RayCaster.render_rays in eval mode).
 *   ray_batch  [n_rays][ray_stride] float: o(3), d(3), near, far (, viewdirs...) — ray_stride >= 8
 *   skts       [n_poses][NJ][4][4]  world->joint transforms
 *   cyls       [n_poses][5]         bounding cylinder (cx, cz, r, top, bot)
 *   ray_pose   [n_rays] int32 pose index per ray, or NULL (all rays use pose 0)
 *   cams       [n_rays] float framecode index per ray (float, truncated like .long()), or NULL;
 *              a negative index selects the eval-mode mean code (core/networks/embedding.py:23-24)
 *   chunk      NaN-fill granularity in rays (the caller's batchify chunk, 4096 in the configs)
 *   outputs: rgb [n][3], disp [n], acc [n]; rgb0/disp0/acc0 (coarse, only when n_importance>0),
 *            alpha [n][S+I or S], alpha0 [n][S] — any optional output may be NULL
 */
int anerf_render_rays(const anerf_model* m, const float* ray_batch, int32_t ray_stride, int64_t n_rays,
                      const float* skts, const float* cyls, int32_t n_poses, const int32_t* ray_pose,
                      const float* cams, int32_t n_samples, int32_t n_importance, int32_t chunk,
                      int32_t precision, float* rgb, float* disp, float* acc, float* rgb0, float* disp0,
                      float* acc0, float* alpha, float* alpha0, const anerf_debug* debug, void* workspace,
                      size_t workspace_bytes, void* stream);

/* Ray batch [n][11] (o, d, near, far, viewdir) for pixel indices idx (y*W + x) of one camera
 * (get_rays at ray_utils.py:6-28 + the gather at :132 + render's batch at core/trainer.py:116-135). */
int anerf_gen_rays(const float* c2w /*3x4 row-major, device*/, int32_t H, int32_t W, float focal_x,
                   float focal_y, float center_x, float center_y, int32_t has_center, const int64_t* idx,
                   int64_t n, float near, float far, float* ray_batch_out, void* stream);

/* Frame compose of render_path (run_nerf.py:100-141): pixels outside idx get the background
 * (bg [hw][3] if given, else 1 when white_bkgd, else 0), disp 0, acc 0; pixels idx[i] get
 * rgb + (1 - acc) * background, disp (NaN -> 0) and acc.  out_acc may be NULL. */
int anerf_compose(const float* rgb, const float* disp, const float* acc, const int64_t* idx, int64_t n,
                  const float* bg, int32_t white_bkgd, int64_t hw, float* out_rgb, float* out_disp, float* out_acc,
                  void* stream);

/* anerf_gen_rays over the pixels of kp_to_valid_rays' box, y in [y0, y1), x in [x0, x1), row-major
 * (the valid_idx order; ray_utils.py:127-130): n = (x1 - x0)(y1 - y0) rays, no index list. */
int anerf_gen_rays_box(const float* c2w, int32_t H, int32_t W, float focal_x, float focal_y, float center_x,
                       float center_y, int32_t has_center, int32_t x0, int32_t y0, int32_t x1, int32_t y1, float near,
                       float far, float* ray_batch_out, void* stream);

/* anerf_compose for rays produced by anerf_gen_rays_box (same box, same order). */
int anerf_compose_box(const float* rgb, const float* disp, const float* acc, int32_t x0, int32_t y0, int32_t x1,
                      int32_t y1, const float* bg, int32_t white_bkgd, int32_t H, int32_t W, float* out_rgb,
                      float* out_disp, float* out_acc, void* stream);

/* Stage: near/far of get_near_far_in_cylinder with the per-chunk NaN fill; cyls [n_poses][5], ray_pose
 * [n_rays] or NULL (pose 0); a ray whose pose index is outside [0, n_poses) is treated as a miss. */
int anerf_near_far(const float* ray_batch, int32_t ray_stride, int64_t n_rays, const float* cyls, int32_t n_poses,
                   const int32_t* ray_pose, int32_t chunk, float* near_out, float* far_out, void* workspace,
                   size_t workspace_bytes, void* stream);

/* Stage: MLP input features [M][F] of points pts [M][3] on rays with directions dirs [M][3],
 * joint transforms skts [NJ][4][4]; F = NJ(1+2 multires) + 3NJ + 3NJ(1+2 multires_views). */
int anerf_encode_points(const anerf_model* m, const float* skts, const float* pts, const float* dirs,
                        int64_t n_points, float* feat_out, void* stream);

/* Raw density (alpha_linear output, before the density activation) of the trunk of one network at
 * points pts [n][3] in world space, one pose skts [NJ][4][4]: _get_density_fwd_fn's fwd_fn.
 * net: 0 coarse, 1 fine, -1 the reference's default (fine if the model has one); precision ANERF_PREC_*. */
int anerf_density_points(const anerf_model* m, const float* pts, int64_t n_points, const float* skts, int32_t net,
                         int32_t precision, float* raw_out, void* stream);

/* The same on render_mesh_density's grid, generated on the device: raw_out [res1][res1][res1],
 * element (a, b, c) at (axis[b], axis[a], axis[c]) + kp0 (numpy 'xy' meshgrid order), where
 * axis [res1] = float32(linspace(-radius, radius, res1)) and kp0 [3] = kps[0, 0]. */
int anerf_density_grid(const anerf_model* m, const float* axis, int32_t res1, const float* kp0, const float* skts,
                       int32_t net, int32_t precision, float* raw_out, void* stream);

/* ABI 20: the iso-surface of a float grid [n0][n1][n2] (element (i, j, k) at grid[(i n1 + j) n2 + k]) as an
 * indexed triangle mesh -- mcubes.marching_cubes of run_render.render_mesh (run_render.py:983-984), on the
 * device.  A sample is inside when value >= threshold (a NaN is outside).  flags:
 *   ANERF_ISO_RELU  samples are clamped at 0 as they are read (render_mesh's np.maximum(raw_d, 0)): this moves
 *                   the vertices, not only the classification;
 *   ANERF_ISO_FLIP  reversed winding (by default normals point from inside to outside, dense to empty).
 * One vertex per sign-changing grid edge, owned by the edge's lower grid point p and its axis, at
 * p + t e_axis, t = (threshold - a) / (b - a) in fp32 (a: the value at p, b: at p + e_axis), in array-index
 * coordinates (axis 0, 1, 2).  Vertices are ordered by (p's linear index, axis); triangles (int32 vertex ids,
 * cases of csrc/anerf_iso_table.inc) by (cell's linear index, table order): the arrays are the same on every run.
 * A dimension of 1 is valid and gives an empty mesh (no cells: no triangles, and no vertices either).
 *
 * anerf_isosurface_workspace: bytes of the scratch both calls share (0, with a message, for invalid dimensions).
 * anerf_isosurface_count: counts into totals_dev (device, int64 [2]: vertices V, triangles T) and leaves the
 * block offsets in ws.  The caller reads the 16 bytes of totals (the one synchronisation), allocates, and calls
 * anerf_isosurface_emit with the SAME grid, dimensions, threshold, relu flag and ws: vertices float [V][3],
 * triangles int32 [T][3].  max_vertices / max_triangles are the arrays' capacities in rows (in [0, 2^31); an
 * output may be NULL where its capacity is 0): no store goes past them, rows beyond them are dropped.
 * Both are allocation-free and asynchronous on `stream`.  ANERF_EINVAL, before any HIP call, for NULL pointers,
 * a dimension < 1, n0 n1 n2 >= 2^31, unknown flag bits, a workspace not 8-byte aligned; ANERF_EWORKSPACE for a
 * workspace smaller than anerf_isosurface_workspace's. */
enum { ANERF_ISO_RELU = 1, ANERF_ISO_FLIP = 2 };
size_t anerf_isosurface_workspace(int32_t n0, int32_t n1, int32_t n2);
int anerf_isosurface_count(const float* grid, int32_t n0, int32_t n1, int32_t n2, float threshold, int32_t flags,
                           void* ws, size_t ws_bytes, int64_t* totals_dev, void* stream);
int anerf_isosurface_emit(const float* grid, int32_t n0, int32_t n1, int32_t n2, float threshold, int32_t flags,
                          void* ws, size_t ws_bytes, float* vertices, int64_t max_vertices, int32_t* triangles,
                          int64_t max_triangles, void* stream);

/* ABI 21: vertex normals of the same mesh.  Call after anerf_isosurface_count with the SAME grid, dimensions,
 * threshold, flags and ws, like anerf_isosurface_emit (before or after it: the pass reads the count pass's
 * block offsets only and writes nothing to ws).  Row v of normals [V][3] belongs to vertex v of
 * anerf_isosurface_emit: same order, same capacity rule (no store past max_vertices rows, rows beyond dropped;
 * capacity 0: no launch), same argument checks.  The contract, shared with isosurface.isosurface_reference
 * (all arithmetic fp32, separately rounded):
 *   values    as read: relu-clamped under ANERF_ISO_RELU, a NaN stays a NaN;
 *   gradient  at a grid point q along axis a: interior (f[q + e_a] - f[q - e_a]) * 0.5f, first row
 *             f[q + e_a] - f[q], last row f[q] - f[q - e_a]; no index ever leaves the grid;
 *   vertex    owned by (p, axis) with the emit pass's t: G = g(p) + t * (g(p + e_axis) - g(p)) per component;
 *   normal    n = -G / sqrtf((Gx*Gx + Gy*Gy) + Gz*Gz), pointing from dense to empty, negated under
 *             ANERF_ISO_FLIP so that it always agrees with the winding; n = (0, 0, 0) where G is zero or not
 *             finite in any component (precisely: unless 0 < the squared length < inf, which also covers a
 *             squared length that underflows to 0 or overflows). */
int anerf_isosurface_normals(const float* grid, int32_t n0, int32_t n1, int32_t n2, float threshold, int32_t flags,
                             const void* ws, size_t ws_bytes, float* normals, int64_t max_vertices, void* stream);

/* ABI 22: the connected components of an indexed triangle mesh (triangles int32 [n_tri][3], vertex ids in
 * [0, n_vertices)) -- what the reference leaves to trimesh's split() on the host, for dropping the detached blobs
 * ("floaters") and cavity surfaces of a noisy density's iso-surface.  Two vertices are in one component iff a chain
 * of triangle edges links them; a vertex no triangle uses is a component of its own with 0 triangles.
 *   root [n_vertices]        the SMALLEST vertex id of the vertex's component (root[r] == r marks a component);
 *   tri_count [n_vertices]   at r == root[r] the component's triangles (a triangle belongs to the component of its
 *                            first vertex), 0 elsewhere;
 *   vert_count [n_vertices]  at r == root[r] the component's vertices, 0 elsewhere;
 *   n_components             device, one int64: the number of components.
 * A lock-free union-find over the triangle list (the larger root hooked under the smaller, so the result does not
 * depend on the schedule) and integer tallies: the outputs are the same on every run.  Precondition: ids lie in
 * [0, n_vertices); a triangle with an id outside is skipped by every kernel (it links nothing and is counted
 * nowhere), so a bad list cannot write out of bounds.  n_tri == 0 and n_vertices == 0 are valid (an array may be
 * NULL where its extent is 0).  ws: anerf_mesh_components_workspace(n_vertices, n_tri) bytes, 4-byte aligned
 * (the size query returns 0, with a message, for counts outside [0, 2^31), and 0 for n_vertices == 0).
 * Allocation-free, asynchronous on `stream`.  ANERF_EINVAL, before any HIP call, for a count outside [0, 2^31), a
 * NULL pointer with a non-zero extent, a NULL n_components, a short or misaligned workspace. */
size_t anerf_mesh_components_workspace(int64_t n_vertices, int64_t n_tri);
int anerf_mesh_components(const int32_t* triangles, int64_t n_tri, int64_t n_vertices, int32_t* root, int32_t* tri_count,
                          int32_t* vert_count, int64_t* n_components, void* ws, size_t ws_bytes, void* stream);

/* ABI 22: stable compaction of such a mesh under a vertex mask keep uint8 [n_vertices]: a vertex survives iff
 * keep[v] != 0, a triangle iff all three of its vertices do (a triangle with an id outside [0, n_vertices) never).
 * Both outputs keep their original relative order (count -> scan -> emit, no atomics):
 *   vertex_map [n_vertices]       the vertex's new id, or -1;
 *   kept [V']                     the surviving vertices' old ids, ascending (the gather index of every per-vertex
 *                                 array: positions, normals, colours);
 *   triangles_out [T'][3]         the surviving triangles, ids through vertex_map.
 * anerf_mesh_compact_count writes totals_dev (device, int64 [2]: V', T') and leaves the block offsets in ws; the
 * caller reads the 16 bytes (the one synchronisation), allocates, and calls anerf_mesh_compact_emit with the SAME
 * keep, lists and ws.  max_kept / max_triangles are the capacities in rows (in [0, 2^31); an output may be NULL
 * where its capacity is 0): no store goes past them, rows beyond them are dropped.  ws:
 * anerf_mesh_compact_workspace(n_vertices, n_tri) bytes, 8-byte aligned (never 0 for valid counts: empty lists
 * still get their totals; 0, with a message, for counts outside [0, 2^31)).  Allocation-free, asynchronous on
 * `stream`.  ANERF_EINVAL, before any HIP call, for a count or capacity outside [0, 2^31), a NULL pointer with a
 * non-zero extent, a NULL or misaligned or short workspace. */
size_t anerf_mesh_compact_workspace(int64_t n_vertices, int64_t n_tri);
int anerf_mesh_compact_count(const uint8_t* keep, int64_t n_vertices, const int32_t* triangles, int64_t n_tri, void* ws,
                             size_t ws_bytes, int64_t* totals_dev, void* stream);
int anerf_mesh_compact_emit(const uint8_t* keep, int64_t n_vertices, const int32_t* triangles, int64_t n_tri,
                            const void* ws, size_t ws_bytes, int32_t* vertex_map, int32_t* kept, int64_t max_kept,
                            int32_t* triangles_out, int64_t max_triangles, void* stream);

/* ABI 23: the vertex adjacency of such a mesh as a CSR.  Every triangle (a, b, c) lists the ordered pairs (a,b) (a,c)
 * (b,a) (b,c) (c,a) (c,b); pairs with equal ends are dropped.  Row v is the set of distinct u with (v,u) listed,
 * ascending; a vertex no triangle uses has an empty row:
 *   offsets [n_vertices + 1]   row v is neighbors[offsets[v] .. offsets[v + 1]);
 *   neighbors [E]              the rows, one after the other;
 *   boundary [n_vertices]      1 iff some (v,u) is listed exactly once (an edge with one triangle on it), else 0: a
 *                              duplicated triangle, or a degenerate one such as (1,1,3), lists its pairs twice.
 * All outputs are integers and the same on every run.  anerf_mesh_adjacency_count writes offsets, boundary and
 * totals_dev (device, int64 [2]: E, the largest distinct degree) and leaves the sorted rows in ws; the caller reads
 * E (the one synchronisation), allocates, and calls anerf_mesh_adjacency_emit with the SAME n_vertices, ws and
 * offsets.  max_neighbors is the capacity in entries (in [0, 2^31); neighbors may be NULL where it is 0): no store
 * goes past it, entries beyond it are dropped.  Rows are counted and filled with integer atomics, sorted (a row of
 * up to 64 listed pairs by one thread, a longer one by a workgroup's bitonic network) and their distinct entries
 * taken from the runs; no kernel waits for another workgroup.  Precondition: ids lie in [0, n_vertices); a triangle
 * with an id outside is skipped by every kernel, so a bad list cannot write out of bounds.  n_tri == 0 and
 * n_vertices == 0 are valid (triangles and boundary may be NULL where their extent is 0; offsets[0] is written
 * always).  ws: anerf_mesh_adjacency_workspace(n_vertices, n_tri) bytes, 4-byte aligned (never 0 for valid counts;
 * 0, with a message, for n_vertices outside [0, 2^31) or 6 n_tri >= 2^31).  Allocation-free, asynchronous on `stream`.
 * ANERF_EINVAL, before any HIP call, for such counts, a capacity outside [0, 2^31), a NULL pointer with a non-zero
 * extent, a NULL or misaligned or short workspace (emit can only tell that the part before the rows is missing: it
 * never reads past ws_bytes). */
size_t anerf_mesh_adjacency_workspace(int64_t n_vertices, int64_t n_tri);
int anerf_mesh_adjacency_count(const int32_t* triangles, int64_t n_tri, int64_t n_vertices, void* ws, size_t ws_bytes,
                               int32_t* offsets, uint8_t* boundary, int64_t* totals_dev, void* stream);
int anerf_mesh_adjacency_emit(int64_t n_vertices, void* ws, size_t ws_bytes, const int32_t* offsets, int32_t* neighbors,
                              int64_t max_neighbors, void* stream);

/* ABI 23: Laplacian / Taubin smoothing of positions [n_vertices][3] over such a CSR (n_neighbors: its E).  One step
 * with weight w, for a vertex v with neighbours u_0 < u_1 < ... < u_{d-1} (its row), d > 0, not pinned, per
 * component, fp32, every operation separately rounded:
 *   s = p[u_0], then s = s + p[u_k] for k = 1 .. d-1 in that order; m = s / (float)d; p'[v] = p[v] + w (m - p[v]);
 * with d == 0 or pinned[v] != 0, p'[v] = p[v] bit for bit.  Every step reads only the previous step's positions
 * (Jacobi, two buffers) and is one launch: a step needs every position of the step before, and no kernel waits for
 * another workgroup.  One iteration is a step with lambda, and under ANERF_SMOOTH_TAUBIN a step with mu after it (mu is
 * ignored without the flag).  NaN and infinity propagate as the arithmetic gives them.  The result lands in `out`
 * whatever the number of steps; `scratch` [n_vertices][3] is the other buffer (may be NULL for fewer than two steps);
 * `positions` is never written.  iterations == 0 copies positions to out.  pinned: uint8 [n_vertices] or NULL (no
 * vertex pinned).  A bad CSR cannot read out of bounds: a row bound outside [0, n_neighbors] is clamped, a neighbour
 * id outside [0, n_vertices) is skipped and not counted in d.  Allocation-free, asynchronous on `stream`.
 * ANERF_EINVAL, before any HIP call, for a count outside [0, 2^31), iterations outside [0, 2^30), unknown flags, a
 * NULL pointer with a non-zero extent, or positions, out and scratch overlapping one another. */
enum { ANERF_SMOOTH_TAUBIN = 1 };
int anerf_mesh_smooth(const float* positions, int64_t n_vertices, const int32_t* offsets, const int32_t* neighbors,
                      int64_t n_neighbors, const uint8_t* pinned, int32_t iterations, float lambda, float mu,
                      int32_t flags, float* out, float* scratch, void* stream);

/* ABI 24: face-accumulated vertex normals of an indexed triangle mesh (vertices float [n_vertices][3], triangles
 * int32 [n_tri][3]) -- compute_normal of the reference's viewer, with every incident face counted (the viewer's own
 * fancy-index add keeps one face per vertex and column).  fp32, every operation separately rounded:
 *   face (a, b, c): e1 = p[b] - p[a], e2 = p[c] - p[a]; n = (e1.y e2.z - e1.z e2.y, e1.z e2.x - e1.x e2.z,
 *   e1.x e2.y - e1.y e2.x); len = sqrt((n.x n.x + n.y n.y) + n.z n.z), raised to 1e-8f when below; n = n / len;
 *   q = (int64) rint(n 2^30) per component (0 for a component that is not finite), added to the 64-bit integer
 *   accumulators of a, b and c -- an integer sum has no order, so the result is the same on every run;
 *   vertex: s = (float) sum 2^-30 (the conversion rounds to nearest even), then the same length, clamp and divide;
 *   a vertex that no triangle uses gets (0, 0, 0).
 * A triangle with an id outside [0, n_vertices) is skipped.  ws: anerf_mesh_vertex_normals_workspace(n_vertices, n_tri)
 * bytes, 8-byte aligned (never 0 for valid counts; 0, with a message, for counts outside [0, 2^31)).
 * Allocation-free, asynchronous on `stream`, no host read.  ANERF_EINVAL, before any HIP call, for a count outside
 * [0, 2^31), a NULL pointer with a non-zero extent, a NULL, misaligned or short workspace. */
size_t anerf_mesh_vertex_normals_workspace(int64_t n_vertices, int64_t n_tri);
int anerf_mesh_vertex_normals(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_tri,
                              float* normals, void* ws, size_t ws_bytes, void* stream);

/* ABI 24: one orthographic (affine) view of such a mesh: per pixel the nearest triangle, its depth, barycentrics and
 * interpolated vertex attributes.  transform: HOST float [3][4], read during the call: for p = (x, y, z)
 * s_i = ((A[i][0] x + A[i][1] y) + A[i][2] z) + A[i][3]; s_0 is pixel x (pixel (row j, column i) has its centre at
 * (i + 0.5, j + 0.5), row 0 at the top), s_1 pixel y downward, s_2 the depth, smaller nearer.
 *   snap      X = (int64) rint(256 s_0), Y likewise; a triangle is dropped whole if any of its nine s is not finite or
 *             an |s_0|, |s_1| exceeds 2^20 (every 64-bit product below then stays under 2^60);
 *   coverage  integers only: with P = (256 i + 128, 256 j + 128), E_ab(P) = (X_b - X_a)(P_y - Y_a) - (Y_b - Y_a)(P_x - X_a),
 *             A2 = E_01(vertex 2); A2 == 0 drops the triangle; A2 < 0 negates A2, E_12, E_20, E_01 and each edge's
 *             (dx, dy) = (X_b - X_a, Y_b - Y_a) (both windings are drawn); covered iff for every edge E > 0, or E == 0
 *             and (dy > 0 or (dy == 0 and dx < 0)): a centre on an edge two triangles share is drawn once;
 *   depth     b1 = (float) E_20 / (float) A2, b2 = (float) E_01 / (float) A2, b0 = (1 - b1) - b2,
 *             z = (b0 z0 + b1 z1) + b2 z2; the fragment is discarded unless 0 <= z <= 1 (a NaN is); -0 counts as +0;
 *             the pixel keeps the smallest key (bits(z) << 32) | triangle id: the nearest, ties to the smaller id (one
 *             64-bit unsigned atomic min per fragment: the result does not depend on the schedule);
 *   resolve   an empty pixel: face_ids -1, depth +inf, bary 0, image = background; else b0, b1, b2 and z again by the
 *             same expressions and image[c] = (b0 a0[c] + b1 a1[c]) + b2 a2[c] over attrs float [n_vertices][n_channels].
 * Outputs (device): face_ids int32 [height][width], depth float [height][width], bary float [height][width][3], image
 * float [height][width][n_channels] (attrs, background (HOST, n_channels floats) and image may be NULL with
 * n_channels == 0).  A triangle whose clipped bounding box holds at most ANERF_RASTER_SMALL_PIXELS pixel centres is
 * rasterised by the thread that set it up, a larger one by workgroups over 64 x 4 tiles of the box, from a list built
 * and read on the device; the outputs are the same bits whichever path it took.  A triangle with an id outside
 * [0, n_vertices) is skipped.  No perspective, no near-plane clipping, no multisampling.
 * ws: anerf_mesh_raster_workspace(n_vertices, n_tri, width, height) bytes, 8-byte aligned (0, with a message, for
 * counts outside [0, 2^31) or a width or height outside [1, 16384]).  One frame per call; allocation-free,
 * asynchronous on `stream`, no host read.  ANERF_EINVAL, before any HIP call and naming the argument, for such counts
 * or sizes, n_channels outside [0, 8], a NULL output, a NULL input with a non-zero extent, a NULL, misaligned or short
 * workspace. */
#define ANERF_RASTER_SMALL_PIXELS 256
size_t anerf_mesh_raster_workspace(int64_t n_vertices, int64_t n_tri, int32_t width, int32_t height);
int anerf_mesh_raster(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_tri,
                      const float* transform, int32_t width, int32_t height, const float* attrs, int32_t n_channels,
                      const float* background, int32_t* face_ids, float* depth, float* bary, float* image, void* ws,
                      size_t ws_bytes, void* stream);

/* ABI 25: vertex clustering (Rossignac-Borrel) of such a mesh: the vertices are snapped to a uniform grid of cells,
 * every cell's vertices become one, and the triangles that collapse or become copies of one another are dropped.
 * Inputs: vertices float [n_vertices][3], triangles int32 [n_tri][3] (device); origin o: HOST float [3]; cell > 0;
 * dims n: HOST int32 [3], every n_a >= 1 and n_0 n_1 n_2 <= ANERF_SIMPLIFY_MAX_CELLS; all read during the call.
 * fp32, every operation separately rounded, divisions correctly rounded:
 *   cell      q_a = (p_a - o_a) / cell, c_a = floor(q_a); the vertex is VALID iff all three q_a are finite and
 *             0 <= c_a < n_a; its key is (c_0 n_1 + c_1) n_2 + c_2;
 *   merge     a cell's representative is its valid member with the smallest vertex id; the new vertices are the
 *             representatives in ascending original id (the relative order is kept, as in anerf_mesh_compact_*):
 *             vertex_map [n_vertices]   the new id of the vertex's cell, or -1 for a vertex that is not valid;
 *             representatives [V']      the original id of new vertex j (the gather index of per-vertex arrays);
 *   position  the fixed-point mean of the cell's members, which has no order: r_a = q_a - (float) c_a (exact),
 *             i_a = (int64) rint(r_a 2^20); S_a = the 64-bit integer sum of i_a over the members, n their number;
 *             m_a = (float) ((double) S_a / (double) n * 2^-20); p'_a = o_a + cell * ((float) c_a + m_a);
 *   triangles (a, b, c) maps to (a', b', c') through vertex_map; it is dropped if an id is outside [0, n_vertices), a
 *             mapped id is -1, two mapped ids are equal, or an earlier surviving triangle (a smaller index) has the
 *             same unordered set {a', b', c'}, in either winding.  The survivors keep their relative order and their
 *             own vertex order: neither rotated nor re-wound.
 * Integers or a fixed order of roundings throughout: the same bits on every run and under any schedule.
 * anerf_mesh_simplify_count writes totals_dev (device, int64 [2]: V', T') and leaves its decisions in ws; the caller
 * reads the 16 bytes (the one synchronisation), allocates, and calls anerf_mesh_simplify_emit with the SAME inputs and
 * ws and with n_out_v = V', n_out_t = T', the rows of out_vertices float [V'][3], representatives [V'] and
 * out_triangles [T'][3] (an output may be NULL where its extent is 0).  The totals live on the device, so the host can
 * refuse only sizes that no count can give (outside [0, n_vertices] / [0, n_tri]); with other sizes no store goes
 * past the sizes given, rows beyond them are dropped.  A vertex that is not valid (a NaN or infinite coordinate among
 * them) and a triangle with an id outside [0, n_vertices) are dropped and never dereferenced.  Representatives by an
 * integer atomic min per vertex into a table over the cells, the sums by 64-bit integer atomic adds; duplicate sets
 * through per-owner rows (the owner: the triangle's smallest representative): a row of up to 32 entries is searched by
 * its triangles' own threads, a longer one sorted by a workgroup's bitonic network; no kernel waits for another
 * workgroup.  n_vertices == 0 and n_tri == 0 are valid (vertices and triangles may be NULL where their extent is 0).
 * ws: anerf_mesh_simplify_workspace(n_vertices, n_tri, n_cells = n_0 n_1 n_2) bytes, 8-byte aligned (never 0 for valid
 * arguments; 0, with a message, for counts outside [0, 2^31) or n_cells outside [1, 2^26]).  Allocation-free,
 * asynchronous on `stream`.  ANERF_EINVAL, before any HIP call, for such counts, a NULL pointer with a non-zero extent,
 * a NULL origin, dims or totals, a cell that is not finite and > 0, an origin that is not finite, a dims entry below 1
 * or a dims product outside [1, 2^26], a NULL, misaligned or short workspace, output sizes outside the ranges above.
 * Out of scope: quadric-error placement, edge-collapse decimation, target triangle counts, keeping the result
 * manifold (clustering can pinch thin parts into edges with more than two triangles). */
#define ANERF_SIMPLIFY_MAX_CELLS (1 << 26)
size_t anerf_mesh_simplify_workspace(int64_t n_vertices, int64_t n_tri, int64_t n_cells);
int anerf_mesh_simplify_count(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_tri,
                              const float* origin, float cell, const int32_t* dims, void* ws, size_t ws_bytes,
                              int64_t* totals_dev, void* stream);
int anerf_mesh_simplify_emit(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_tri,
                             const float* origin, float cell, const int32_t* dims, const void* ws, size_t ws_bytes,
                             float* out_vertices, int64_t n_out_v, int32_t* out_triangles, int64_t n_out_t,
                             int32_t* vertex_map, int32_t* representatives, void* stream);

/* ABI 26: one view of such a mesh through a perspective (pinhole) camera, cut at the near plane: anerf_mesh_raster's
 * outputs, integer coverage, 64-bit atomic-min depth test and small / large split (whose bits do not change), with a
 * camera that can have vertices behind the eye, triangles across the near plane and interpolation that is not linear
 * on the screen.  view: HOST float [3][4]; intrinsics: HOST float fx, fy, cx, cy; both read during the call.  fp32,
 * every operation separately rounded, divisions correctly rounded; every decision is taken on integers or on one
 * comparison of such values.
 *   camera    c_k = ((V[k][0] x + V[k][1] y) + V[k][2] z) + V[k][3] gives (xc, yc, d): xc to the right, yc down the
 *             image, d the distance along the optical axis, positive in front.  A triangle with an id outside
 *             [0, n_vertices), or with any of its nine c not finite, draws nothing.
 *   near      a vertex is IN iff d >= near.  No vertex IN: the triangle draws nothing.  All three IN: one sub-triangle,
 *             the triangle itself (q0 q1 q2 = its vertices in its order).  One or two IN: the triangle is cut into a
 *             polygon of 3 or 4 vertices, walked in the triangle's own vertex order from the IN vertex whose predecessor
 *             is not IN -- with s that vertex, one IN: q = (v_s, cut(s, s+1), cut(s, s+2)); two IN: q = (v_s, v_s+1,
 *             cut(s+1, s+2), cut(s, s+2)) (indices mod 3) -- and fanned from its first vertex into the sub-triangles
 *             (q0 q1 q2) and (q0 q2 q3).  cut(I, O), always from the IN end I to the OUT end O whatever direction
 *             the walk crosses the edge: t = (d_I - near) / (d_I - d_O); xc = xc_I + t (xc_O - xc_I), yc likewise,
 *             d = near exactly -- a function of the two end points alone, so two triangles that share the edge get the
 *             same bits: no cracks.  Every polygon vertex carries a row of weights over the ORIGINAL vertices: a unit
 *             row for an original vertex, 1 - t at I, t at O and 0 at the third for a cut point.
 *   project   per polygon vertex s_0 = fx (xc / d) + cx, s_1 = fy (yc / d) + cy, iw = 1 / d (d >= near > 0).  Pixel
 *             centres, the snap X = (int64) rint(256 s_0), the 2^20 limit, the A2 == 0 rule, both windings, the edge
 *             functions and the tie rule are anerf_mesh_raster's, per sub-triangle.  A triangle with a polygon vertex
 *             whose s_0, s_1 or iw is not finite, or whose |s_0| or |s_1| exceeds 2^20, draws nothing at all; a
 *             sub-triangle with A2 == 0 draws nothing itself.  There is no side-plane or guard-band clipping: a
 *             triangle that reaches beyond 2^20 pixels is dropped, not cut.
 *   fragment  b0, b1, b2: anerf_mesh_raster's screen barycentrics of the sub-triangle; u_k = b_k iw_k,
 *             sum = (u_0 + u_1) + u_2, dep = 1 / sum.  The fragment is discarded unless 0 < dep <= far (a NaN is); near
 *             is not tested again (the cut was the test: dep rounds to either side of near along the cut line).  The
 *             pixel keeps the smallest key (bits(dep) << 32) | ORIGINAL triangle id (one 64-bit unsigned atomic min).
 *   resolve   an empty pixel: anerf_mesh_raster's values.  Else the winning triangle's sub-triangles are tried in
 *             order and the first whose fragment at the centre is kept with bits(dep) equal to the key's gives
 *             g_k = u_k dep, B = (g_0 r_0 + g_1 r_1) + g_2 r_2 per component over its vertices' rows (all nine products
 *             and six sums are taken), image[c] = (B_0 a_0[c] + B_1 a_1[c]) + B_2 a_2[c] over the ORIGINAL vertices.
 * Outputs as anerf_mesh_raster's: face_ids the original triangle id, depth = dep, the camera depth d of the surface
 * there (the parameter of the pixel's ray when its direction has d = 1; not a normalised z), +inf where empty; bary = B,
 * perspective-correct weights over the original vertices; image the attributes under them.  The seam q0-q2 is an edge
 * of both sub-triangles on the same snapped end points, so the tie rule gives a centre on it to one of them, as on an
 * edge between two triangles.  A triangle whose sub-triangles' clipped boxes hold at most ANERF_RASTER_SMALL_PIXELS
 * pixel centres together is drawn by the thread that set it up; a larger one goes onto the list once and its workgroups
 * draw both sub-triangles: the same bits either way, on every run.  No side-plane clipping, no multisampling, no
 * back-face culling.
 * ws: anerf_mesh_raster_persp_workspace(n_vertices, n_tri, width, height) bytes (anerf_mesh_raster_workspace's layout
 * and size), 8-byte aligned.  One frame per call; allocation-free, asynchronous on `stream`, no host read.
 * ANERF_EINVAL, before any HIP call and naming the argument, for anerf_mesh_raster's cases, a NULL view or intrinsics,
 * near not finite or <= 0, far not finite or < near, an intrinsic that is not finite, fx or fy equal to 0. */
size_t anerf_mesh_raster_persp_workspace(int64_t n_vertices, int64_t n_tri, int32_t width, int32_t height);
int anerf_mesh_raster_persp(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_tri,
                            const float* view, const float* intrinsics, float near, float far, int32_t width,
                            int32_t height, const float* attrs, int32_t n_channels, const float* background,
                            int32_t* face_ids, float* depth, float* bary, float* image, void* ws, size_t ws_bytes,
                            void* stream);

/* ABI 21: raw network output at arbitrary points, every point with its own ray direction: raw_out [n][4] =
 * (rgb before the sigmoid, sigma before the density activation), the quantities of anerf_debug.raw_coarse /
 * raw_fine and of the reference's `raw` (core/networks/nerf.py:133-148).  pts [n][3] world points; dirs
 * [n_dirs][3] with n_dirs == n_points, or 1 (one direction for all points).  dirs plays the role of ray_batch
 * columns 3:6 (rays_d) of anerf_render_rays: point i is treated as a sample of a ray with direction i -- the view
 * input of joint j is R_j d, normalised (un-normalised under ANERF_ENC_VIEW_RAW), windowed by the point's own
 * distance to the joint.  skts [NJ][4][4]: one pose.  cam: one framecode index for the call, truncated like
 * .long(); negative: the eval-mode mean code; ignored without framecodes.  net / precision: as
 * anerf_density_points (-1: the reference's default; single_net folds 1 into 0).
 * ANERF_EINVAL, before any HIP call, for a NULL pointer, n_points < 0, n_dirs not in {1, n_points}, an unknown
 * net or precision, a framecode index >= n_framecodes, a staged model; for a model on another device.
 * n_points == 0 returns ANERF_OK without a launch.  No workspace, no allocation, asynchronous on `stream`. */
int anerf_radiance_points(const anerf_model* m, const float* pts, int64_t n_points, const float* dirs, int64_t n_dirs,
                          const float* skts, float cam, int32_t net, int32_t precision, float* raw_out, void* stream);

/* Pose -> skeleton transforms for n_frames frames, replacing
 *   PoseOptLayer.calculate_kinematic  core/pose_opt.py:372-445 (+ unrolled_kinematic_chain :482-521),
 *   get_kinematic_chain_T              core/pose_opt.py:448-479,
 *   get_smpl_l2ws + inv                core/utils/skeleton_utils.py:296-376.
 * bones [F][NJ][rot_dim]: rot_dim 3 axis-angle (pytorch3d axis_angle_to_matrix, skeleton_utils.py:411),
 * 6 the 6-D parameters (rot6d_to_rotmat, :420), 9 row-major 3x3 matrices; rest [n_rest][NJ][3],
 * rest_idx [F] (NULL: rest 0; out-of-range index -> NaN outputs for that frame); pelvis [F][3] or NULL,
 * added to every joint's translation; rest offsets are multiplied by scale.  parents [NJ] (HOST
 * memory, the skeleton's joint_trees; the root's entry is ignored) must form a tree rooted at root_id,
 * in any index order; NJ <= 128.  Outputs (any may be NULL): kps [F][NJ][3], skts = inverse(l2ws)
 * [F][NJ][4][4], l2ws [F][NJ][4][4], rots [F][NJ][3][3].  Computed in float64, stored as float32. */
int anerf_pose_kinematics(const float* bones, int32_t rot_dim, const float* rest, const int32_t* rest_idx,
                          int64_t n_rest, const float* pelvis, float scale, const int32_t* parents, int32_t n_joints,
                          int32_t root_id, int64_t n_frames, float* kps, float* skts, float* l2ws, float* rots,
                          void* stream);

/* Backward of anerf_pose_kinematics (the pose-optimisation gradient: PoseOptLayer's autograd,
 * core/pose_opt.py:372-445 + torch.inverse): with the same inputs and the gradients of its outputs
 * (g_kps [F][NJ][3], g_skts / g_l2ws [F][NJ][4][4], g_rots [F][NJ][3][3]; any may be NULL = zero),
 * writes g_bones [F][NJ][rot_dim] and, when not NULL, g_pelvis [F][3] (overwritten, not accumulated).
 * The chain is recomputed in float64. */
int anerf_pose_kinematics_backward(const float* bones, int32_t rot_dim, const float* rest, const int32_t* rest_idx,
                                   int64_t n_rest, const float* pelvis, float scale, const int32_t* parents,
                                   int32_t n_joints, int32_t root_id, int64_t n_frames, const float* g_kps,
                                   const float* g_skts, const float* g_l2ws, const float* g_rots, float* g_bones,
                                   float* g_pelvis, void* stream);

/* Bounding cylinder and 2-D pixel box of every frame on the device, the host
 * half of kp_to_valid_rays (core/utils/ray_utils.py:83-136): get_kp_bounding_cylinder
 * (skeleton_utils.py:542-592; extend_mm 250, top/bot expand 1.6/1.1, head '-y') of kps [n_kp][NJ][3]
 * (or the given cylinders cyls_in [n_kp][5] when kps is NULL), then cylinder_to_box_2d
 * (skeleton_utils.py:607-694) for frame i with cylinder i % n_kp, extrinsic w2cs [F][4][4] =
 * float32 inv(swap_mat(c2w)) (nerf_c2w_to_extrinsic, computed by the caller as the reference does),
 * focals [F][2] float32 (fx, fy), offsets [F][2] = int(center) or NULL (int(W/2), int(H/2)), cap_dirs [50][2] =
 * float64 (cos, sin) of linspace(0, 2 pi, 50) as numpy computes them (NULL: device cos/sin).
 * Outputs cyls_out [n_kp][5] float32 (optional) and boxes_out [F][4] int32 = (x0, y0, x1, y1):
 * pixels y in [y0, y1), x in [x0, x1) — the integers the reference computes. */
int anerf_kp_boxes(const float* kps, const float* cyls_in, int64_t n_kp, int32_t n_joints, int32_t root_id,
                   double ext_scale, const float* w2cs, const float* focals, const int32_t* offsets, int64_t n_frames,
                   int32_t H, int32_t W, const double* cap_dirs, float* cyls_out, int32_t* boxes_out, void* stream);

/* Training ray batch of the image dataset (the `.h5` ray sampler):
 * BaseH5Dataset.__getitem__ (core/dataset.py:57-105) for n_img images at once in ray_collate_fn's
 * flattened layout (core/dataset.py:796-802), from uint8 images resident on the device.  Inputs (the
 * .h5 arrays): imgs [n_rows][H*W][3], masks [n_rows][H*W] (NULL: fg = 1), bgs [n_bg][H*W][3] with
 * bg_idx [n_rows] (NULL: no backgrounds), c2ws [n_rows][4][4] float32, focals [n_rows] float32,
 * centers [n_rows][2] float32 (NULL: image centre); rows [n_img] = dataset row of each batch image,
 * pixels [n_img][n_per] = its sampled pixel indices y*W + x (drawn by the caller: the reference's
 * numpy RNG, sample_pixels core/dataset.py:277-323).  Outputs: rays_out [2][n][3] (rays_o, rays_d of
 * get_rays :346-364, including its isclose(c2w, I) shortcut), target_out [n][3] (get_img_data
 * :259-275; img * fg + (1 - fg) * bg when mask_img and bgs), fg_out [n] and bg_out [n][3] (optional),
 * n = n_img * n_per.  An out-of-range row, pixel or bg_idx makes that ray's outputs NaN and sets
 * *bad_out = 1 (device int32, may be NULL; the check guards the reads either way). */
int anerf_ray_batch(const uint8_t* imgs, const uint8_t* masks, const uint8_t* bgs, const int64_t* bg_idx,
                    const float* c2ws, const float* focals, const float* centers, int64_t n_rows, int64_t n_bg,
                    int32_t H, int32_t W, const int64_t* rows, int64_t n_img, const int64_t* pixels, int64_t n_per,
                    int32_t mask_img, float* rays_out, float* target_out, float* fg_out, float* bg_out,
                    int32_t* bad_out, void* stream);

/* Per-ray copies of per-image rows (ray_collate_fn's kp3d / bones / skts / cyls, core/dataset.py:
 * 96-104, 796-802: every ray of batch image i carries image i's pose rows): dst [n_img * n_per][width]
 * = src [rows[t / n_per]][width] float32, one launch per array (ABI 12; before, torch index_select).
 * A row outside [0, n_rows) gives NaN rows and sets *bad_out = 1 (device int32, may be NULL). */
int anerf_gather_rows(const float* src, int64_t width, int64_t n_rows, const int64_t* rows, int64_t n_img,
                      int64_t n_per, float* dst, int32_t* bad_out, void* stream);

/* ---- Training stages.  All pointers are device pointers; random numbers are
 * inputs (torch.rand / torch.randn draws of the caller), so a run can reproduce the reference's. */

/* z [N][S] of sample_from_lineseg: linspace(near, far) (torch.linspace's float32 values), then with
 * t_rand [N][S] (NULL: perturb = 0) lower + (upper - lower) t_rand inside the mid-point intervals. */
int anerf_train_samples(const float* near_in, const float* far_in, int64_t n_rays, int32_t n_samples,
                        const float* t_rand, int32_t flags /* ANERF_FLAG_LINDISP or 0 */, float* z_out,
                        void* stream);

/* Features feat_out [N][S][F] (the layout of anerf_encode_points) of the points o + d z of the rays
 * ray_batch [N][ray_stride] (o = cols 0-2, d = cols 3-5) at z [N][S]; the rays' skeletons are
 * skts [n_poses][NJ][4][4] with ray_pose [N] (NULL: one skeleton per ray, n_poses == N).  A ray
 * whose ray_pose is outside [0, n_poses) gets NaN features (and no gradient in the backward); the
 * index is never dereferenced.  pts_noise [N][S][3] (NULL: none) is added to the points, sample_pts'
 * `pts + randn_like(pts) * ray_noise_std` (core/raycasters.py:660-661): pass randn * ray_noise_std. */
int anerf_train_encode(const anerf_model* m, const float* ray_batch, int32_t ray_stride, int64_t n_rays,
                       const float* z, int32_t n_samples, const float* skts, int32_t n_poses, const int32_t* ray_pose,
                       const float* pts_noise, float* feat_out, void* stream);

/* dL/dskts of anerf_train_encode (same z and pts_noise) given dL/dfeat [N][S][F], ACCUMULATED into grad_skts
 * [n_poses][NJ][4][4] (row 3 of every transform untouched; the caller zeroes the buffer). */
int anerf_train_encode_backward(const anerf_model* m, const float* ray_batch, int32_t ray_stride, int64_t n_rays,
                                const float* z, int32_t n_samples, const float* skts, int32_t n_poses,
                                const int32_t* ray_pose, const float* pts_noise, const float* grad_feat,
                                float* grad_skts, void* stream);

/* raw2outputs of raw [N][S][4] at z [N][S] with noise [N][S] (= randn * raw_noise_std * B, added to
 * raw_sigma / B; NULL: none): rgb [N][3], disp [N], acc [N], weights, alpha and the exclusive
 * transmittance trans [N][S] (kept for the backward).  S <= 1024 (one wave per ray, LDS-staged), and no S whose
 * BACKWARD would not fit the 64 KB of dynamic LDS (9 S floats): ANERF_EINVAL before any launch, so a forward that
 * succeeds has a backward that can run. */
int anerf_train_composite(const anerf_model* m, const float* raw, const float* z, const float* ray_batch,
                          int32_t ray_stride, int64_t n_rays, int32_t n_samples, const float* noise, float* rgb,
                          float* disp, float* acc, float* weights, float* alpha, float* trans, void* stream);

/* g_raw [N][S][4] from the gradients of the outputs of anerf_train_composite (g_rgb [N][3], g_disp,
 * g_acc [N], g_weights, g_alpha [N][S]; any may be NULL = zero) and its saved weights/alpha/trans;
 * S <= 1024. */
int anerf_train_composite_backward(const anerf_model* m, const float* raw, const float* z, const float* ray_batch,
                                   int32_t ray_stride, int64_t n_rays, int32_t n_samples, const float* noise,
                                   const float* weights, const float* alpha, const float* trans, const float* g_rgb,
                                   const float* g_disp, const float* g_acc, const float* g_weights,
                                   const float* g_alpha, float* g_raw, void* stream);

/* z_all [N][S+I] (sorted) of isample_from_lineseg: sample_pdf over the mid-points with the coarse
 * weights [N][S] at u [N][I] (NULL: det=True, torch.linspace), merged with z [N][S].  single_net != 0
 * uses is_only's weights 0.5 (max(w_l, w_k) + max(w_k, w_u)) + 0.01 (ray_utils.py:270-277).
 * sorted_idx [N][S+I] (optional): torch.sort's indices into cat([z, z_samples]) (ties: values equal). */
int anerf_train_importance(const float* z, const float* weights, int64_t n_rays, int32_t n_samples,
                           int32_t n_importance, const float* u, int32_t single_net, float* z_all,
                           int32_t* sorted_idx, void* stream);

/* The view-window layout's per-ray view factors (ABI 16, ANERF_ENC_VIEW_WINDOWS): G [N][NJ][width] with
 * G[r][j][h] = sum_{f, c} T_fc(e_rj) weight[h ld_weight + f 3 NJ + 3 j + c] col_scale[f 3 NJ + 3 j + c], e_rj = R_j d_r
 * normalised (R_j d_r itself under ANERF_ENC_VIEW_RAW), T_0c = e_c, T_{2m+1,c} / T_{2m+2,c} = sin / cos (2^m e_c),
 * m < multires_views: joint j's view features without their window (encode_inputs' view part,
 * core/raycasters.py:476-555, core/encoders.py:172-193).  weight points at the view layer's first view column
 * (views_linears.0.weight + W, row stride ld_weight); col_scale (the --freq_schedule weights of the view columns) may
 * be NULL.  Skeletons as anerf_train_encode (ray_pose NULL: one per ray).  width <= 128; not for ray-angle views. */
int anerf_train_view_factor(const anerf_model* m, const float* ray_batch, int32_t ray_stride, int64_t n_rays,
                            const float* skts, int32_t n_poses, const int32_t* ray_pose, const float* weight,
                            int64_t ld_weight, int32_t width, const float* col_scale, float* G, void* stream);
/* Its gradients from grad_G: ADDED into grad_skts [n_poses][NJ][4][4] (the rotation blocks, atomically) and into
 * grad_weight (the view columns, the same layout as weight; no other writer on the stream meanwhile).  workspace:
 * device scratch of anerf_train_view_factor_workspace() bytes (16-byte aligned; the per-workgroup partial sums of the
 * weight gradient, reduced in order by a second launch). */
size_t anerf_train_view_factor_workspace(int64_t n_rays, int32_t n_joints, int32_t multires_views, int32_t width);
int anerf_train_view_factor_backward(const anerf_model* m, const float* ray_batch, int32_t ray_stride, int64_t n_rays,
                                     const float* skts, int32_t n_poses, const int32_t* ray_pose, const float* weight,
                                     int64_t ld_weight, int32_t width, const float* col_scale, const float* grad_G,
                                     float* grad_skts, float* grad_weight, void* workspace, size_t workspace_bytes,
                                     void* stream);

/* The view-window layout's view part (ABI 16, ANERF_ENC_VIEW_WINDOWS): out [N S][width] = sum_j w_j G_j, the NJ
 * windows w of sample s of ray r at windows + (r S + s) ld_windows (the window columns of an anerf_train_encode
 * row) and G [N][NJ][width] the ray's view factors (the view layer's view columns times the ray's direction
 * terms, per joint).  width % 4 == 0, G and out 16-byte aligned; G and a chunk of windows are staged in LDS:
 * 4 (NJ width + 32 NJ) bytes <= 64 KB here, 4 (4 ceil(NJ / 4) (width + 4) + 32 (width + 4) + 32 NJ) bytes in
 * the backward, which also keeps dL/dG in registers: NJ width <= 9216 (width 128: NJ <= 72; ANERF_EINVAL
 * beyond).  In the reference this is
 * part of views_linears.0's product with the view features (core/networks/nerf.py:141-148). */
int anerf_train_view_mix(int64_t n_rays, int32_t n_samples, int32_t n_joints, int32_t width, const float* windows,
                         int64_t ld_windows, const float* G, float* out, void* stream);
/* Its gradients from grad_out [N S][width]: grad_windows (r S + s) ld_grad_windows + j = sum_h grad_out G_j (written),
 * grad_G [N][NJ][width] = sum_s w_j grad_out (written). */
int anerf_train_view_mix_backward(int64_t n_rays, int32_t n_samples, int32_t n_joints, int32_t width,
                                  const float* windows, int64_t ld_windows, const float* G, const float* grad_out,
                                  float* grad_windows, int64_t ld_grad_windows, float* grad_G, void* stream);

/* ---- training MLP linears on the bf16 MFMA pipe, fp32 in / out with split-bf16 operands:
 *   ANERF_MLP_BF16X6  x = x0 + x1 + x2, w likewise, the six products with i + j <= 2 (fp32-accurate:
 *                     the dropped terms are below 2^-23 of |x w|), fp32 accumulation
 *   ANERF_MLP_BF16X3  x = x0 + x1, three products (~16 significant bits per operand)
 *   ANERF_MLP_FP16X4  forward products only (anerf_mlp_gemm_rows): each A row scaled by a power of two
 *                     from its largest |value| (row maxima given), the weights by one from theirs
 *                     (computed on the device by the split), x = x0 + x1 and w = w0 + w1 in fp16, all
 *                     four products on v_mfma_f32_32x32x16_f16: within ~2^-22 of |x w| per product, the
 *                     bound of ANERF_MLP_BF16X6 (the render path's fp16x4) */
enum { ANERF_MLP_BF16X3 = 3, ANERF_MLP_FP16X4 = 4, ANERF_MLP_BF16X6 = 6 };
/*
 * An operand is up to 3 column segments (the reference's torch.cat along features, never
 * materialised here): segment i holds columns [sum of earlier cols, + cols) at p[row * ld + c]. */
typedef struct {
    const float* p;
    int64_t ld;    /* row stride in floats (>= cols) */
    int32_t cols;
} anerf_seg;

/* An output column segment: out[row * ld + c] = v, v *= (mask[row * ldm + c] > 0) when mask is set
 * (relu backward by the saved activation), v += out[...] when accumulate == 1 (after the relu and mask);
 * accumulate == 2 (ABI 16) adds out[...] to the pre-activation instead (product + bias + out, then the relu: the
 * view-window layout's view part, anerf_train_view_mix); p NULL discards it. */
typedef struct {
    float* p;
    int64_t ld;
    int32_t cols;
    const float* mask;
    int64_t ldm;
    int32_t accumulate;
} anerf_oseg;

/* The training MLP's forward as ONE fused kernel (mlp.py with ANERF_TRAIN_FWD=fused, widths 128 /
 * 256, bf16x6 forward; measured equal to the layer GEMMs): NeRF.forward
 * (core/networks/nerf.py:94-148) over M rows of encoder features, every layer's output written once
 * for the backward.  feat [m][ld_feat]: x = columns [0, dnet),
 * views = [dnet, dnet + nv); codes [m][ld_codes] (cfc columns) or NULL.  Outputs: h[i] [m][W] =
 * relu(pts_linears[i](.)), hf [m][W] = feature_linear(h[D-1]), g [m][W/2] = relu(views_linears.0(
 * [hf | views | codes])), raw [m][4] = [rgb_linear(g), alpha_linear(h[D-1])].  Arithmetic as
 * ANERF_MLP_BF16X6.  The weights are packed once per step (anerf_mlp_forward_pack, one launch). */
typedef struct {
    int32_t depth, width;  /* width 128 or 256 */
    int32_t skip;          /* pts_linears[skip + 1] takes [x | h]; -1 (or >= depth - 1): none */
    int32_t dnet, nv, cfc; /* multiples of 4; cfc 0: no framecodes */
} anerf_mlp_shape;
typedef struct {
    const float* pts_w[16]; /* pts_linears[i].weight [W][in] */
    int64_t pts_ld[16];
    const float* feature_w; /* [W][W] */
    const float* views_w;   /* views_linears.0.weight [W/2][W + nv + cfc] */
    int64_t views_ld;
} anerf_mlp_fwd_weights;
typedef struct {
    int64_t m;
    const float* feat;
    int64_t ld_feat;
    const float* codes;
    int64_t ld_codes;
    const float* pts_b[16];
    const float* feature_b;
    const float* alpha_w; /* [W] */
    const float* alpha_b; /* [1] (device) */
    const float* views_b; /* [W/2] */
    const float* rgb_w;   /* [3][W/2] */
    const float* rgb_b;   /* [3] */
    float* h[16];
    float* hf;
    float* g;
    float* raw;
} anerf_mlp_fwd_io;
size_t anerf_mlp_forward_pack_bytes(const anerf_mlp_shape* s);
int anerf_mlp_forward_pack(const anerf_mlp_shape* s, const anerf_mlp_fwd_weights* w, void* packed, void* stream);
int anerf_mlp_forward(const anerf_mlp_shape* s, const anerf_mlp_fwd_io* io, const void* packed, void* stream);

/* Bytes of one split operand of `rows` x `cols` (anerf_mlp_split_weights' output). */
size_t anerf_mlp_split_bytes(int32_t rows, int32_t cols, int32_t precision);
/* w [n][k] (row stride ldw) -> bf16 planes (hi, then lo), zero padded; transpose != 0 splits w^T
 * ([k][n], the B operand of an input gradient).  out: anerf_mlp_split_bytes(rows, cols) bytes. */
int anerf_mlp_split_weights(const float* w, int32_t n, int32_t k, int64_t ldw, int32_t transpose,
                            int32_t precision, void* out, void* stream);
/* One anerf_mlp_split_weights call of a batch. */
typedef struct {
    const float* w;
    int32_t n, k;
    int64_t ldw;
    int32_t transpose, precision;
    void* out;
} anerf_split_job;
/* Up to 32 anerf_mlp_split_weights in one launch (a network's layers: forward or transposed). */
int anerf_mlp_split_weights_batch(const anerf_split_job* jobs, int32_t n_jobs, void* stream);
/* C[m][n] = act(sum_k A[m][k] B[n][k] + bias[n]); A: n_a segments adding up to k columns; B: split
 * [n][k] (the forward's weight, or the transposed weight of an input gradient); bias NULL or [n];
 * relu != 0 applies max(., 0); C: n_c segments adding up to n columns. */
int anerf_mlp_gemm(int64_t m, int32_t n, int32_t k, const anerf_seg* a, int32_t n_a, const void* b_split,
                   int32_t precision, const float* bias, int32_t relu, const anerf_oseg* c, int32_t n_c,
                   void* stream);
/* anerf_mlp_gemm with row maxima: rowmax_in [m] (ANERF_MLP_FP16X4 only, required there; one A segment):
 * the bit patterns of max_k |A[row][k]| (as written by rowmax_out); rowmax_out [m] (NULL or any
 * precision, n % 128 == 0, zeroed by the caller): atomically max'd with the bit patterns of
 * max_j |C[row][j]| after bias and relu (the next layer's rowmax_in).  The split weights of
 * ANERF_MLP_FP16X4 carry their exponent (anerf_mlp_split_bytes includes it). */
int anerf_mlp_gemm_rows(int64_t m, int32_t n, int32_t k, const anerf_seg* a, int32_t n_a, const void* b_split,
                        int32_t precision, const float* bias, int32_t relu, const anerf_oseg* c, int32_t n_c,
                        const int32_t* rowmax_in, int32_t* rowmax_out, void* stream);
/* Workspace bytes of anerf_mlp_wgrad for these sizes. */
size_t anerf_mlp_wgrad_workspace(int64_t m, int32_t n, int32_t k);
/* dW[n][k] (+)= sum_m dY[m][n] X[m][k] and db[n] (+)= sum_m dY[m][n] (db may be NULL); X: n_x
 * segments adding up to k columns.  Summed over row slabs in a fixed order (deterministic).  dY is
 * read in 4-column groups: 16 B aligned, lddy % 4 == 0, lddy >= round_up(n, 4) (columns n.. of the
 * last group are read but reach no output). */
int anerf_mlp_wgrad(int64_t m, int32_t n, int32_t k, const float* dy, int64_t lddy, const anerf_seg* x, int32_t n_x,
                    int32_t precision, float* dw, int64_t lddw, float* db, int32_t accumulate, void* workspace,
                    size_t workspace_bytes, void* stream);

/* Workspace bytes of anerf_mlp_backward_hidden (0 for an unsupported width). */
size_t anerf_mlp_backward_hidden_workspace(int64_t m, int32_t width);
/* The backward of one hidden layer y = relu(x W^T + b) of width 256 (pts_linears[i], i not after the skip,
 * core/networks/nerf.py:133-139; its autograd in the reference), from its pre-activation gradient dy [m][256]
 * and its input x [m][256] (the previous layer's relu output), in ONE pass over both:
 *   dx[m][i] = (sum_o dy[m][o] W[o][i]) if x[m][i] > 0 else 0    (the input gradient, relu' masked by x)
 *   dw[o][i] = sum_m dy[m][o] x[m][i],  db[o] = sum_m dy[m][o]    (written, not accumulated)
 * wt_split: W's transposed planes from anerf_mlp_split_weights(W, 256, 256, ld, transpose 1, precision).
 * precision: ANERF_MLP_BF16X3 (the "mixed" mode's backward arithmetic, as anerf_mlp_gemm / _wgrad).  The
 * same sums as anerf_mlp_gemm (input gradient with the relu' mask) + anerf_mlp_wgrad in another summation order;
 * deterministic (per-workgroup slabs summed in order).  dy, x: 16 B aligned, ld % 4 == 0, 256 <= ld < 2^22.
 * dw = db = NULL: the weight and bias gradients stay as slabs in the workspace for a later
 * anerf_mlp_backward_hidden_reduce (on another stream, beside the next layer's pass). */
int anerf_mlp_backward_hidden(int64_t m, int32_t width, const float* dy, int64_t lddy, const float* x, int64_t ldx,
                              const void* wt_split, int32_t precision, float* dx, int64_t lddx, float* dw, int64_t lddw,
                              float* db, void* workspace, size_t workspace_bytes, void* stream);
/* dw, db of an anerf_mlp_backward_hidden call made with dw = db = NULL, from its workspace (same m, width). */
int anerf_mlp_backward_hidden_reduce(int64_t m, int32_t width, const void* workspace, size_t workspace_bytes, float* dw,
                                     int64_t lddw, float* db, void* stream);

/* Workspace bytes of anerf_mlp_backward_head (0 for an unsupported width). */
size_t anerf_mlp_backward_head_workspace(int64_t m, int32_t width);
/* ABI 18: the backward of the heads on the last hidden layer's output x [m][256] -- feature_linear (256 x 256) and
 * alpha_linear (1 x 256), core/networks/nerf.py:141-145 (the reference runs them as two nn.Linear; here, as in the
 * forward, one [257][256] weight, feature rows then alpha's) -- in ONE pass over dy and x, as
 * anerf_mlp_backward_hidden:
 *   dx[m][i] = (sum_o dy[m][o] Wf[o][i] + dy[m][256] w_alpha[i]) if x[m][i] > 0 else 0
 *   dw[o][i] = sum_m dy[m][o] x[m][i] for o < 257 (row 256: alpha's), db[o] = sum_m dy[m][o] (257 entries)
 * dy rows hold the 256 feature gradients then alpha's at column 256 (lddy >= 257, % 4 == 0); wt_split: Wf's
 * transposed bf16x3 planes (anerf_mlp_split_weights(Wf, 256, 256, ld, 1, ANERF_MLP_BF16X3)); w_alpha [256] fp32.
 * Feature part in bf16x3 (as anerf_mlp_backward_hidden), alpha's terms in fp32.  dw [257][lddw], db [257], or
 * both NULL for a later anerf_mlp_backward_head_reduce. */
int anerf_mlp_backward_head(int64_t m, int32_t width, const float* dy, int64_t lddy, const float* x, int64_t ldx,
                            const void* wt_split, const float* w_alpha, int32_t precision, float* dx, int64_t lddx,
                            float* dw, int64_t lddw, float* db, void* workspace, size_t workspace_bytes, void* stream);
/* dw [257][lddw], db [257] of an anerf_mlp_backward_head call made with dw = db = NULL (same m, width). */
int anerf_mlp_backward_head_reduce(int64_t m, int32_t width, const void* workspace, size_t workspace_bytes, float* dw,
                                   int64_t lddw, float* db, void* stream);

/* ABI 19: the forward of one hidden layer of width 256 (pts_linears[i], core/networks/nerf.py:133-139),
 *   y[m][o] = relu(sum_i x[m][i] W[o][i] + b[o]),
 * bit-identical to anerf_mlp_gemm(m, 256, 256, {x}, w_split, precision, b, relu 1, {y}) -- the same split, the same
 * products in the same order -- on one persistent workgroup per CU whose stager waves stream x from HBM and the
 * output tile back while its compute waves run the MFMAs (anerf_gemm.hip, mlp_fwd_kernel).  w_split:
 * anerf_mlp_split_weights(W, 256, 256, ld, transpose 0, precision); precision ANERF_MLP_BF16X6 or _BF16X3.
 * x, y: 16 B aligned rows, ld % 4 == 0, 256 <= ld < 2^22; y must not overlap x. */
int anerf_mlp_forward_hidden(int64_t m, int32_t width, const float* x, int64_t ldx, const void* w_split,
                             int32_t precision, const float* bias, float* y, int64_t ldy, void* stream);
/* ABI 19: the same persistent kernel for any layer with 256 outputs on k > 128 input columns (k % 4 == 0) given as
 * one or two operand segments (layer 0 on the encoder features, the skip layer on [x | h]; each segment 16 B aligned,
 * cols % 4 == 0, cols <= ld < 2^22, ld % 4 == 0):  y[m][o] = act(sum_i a[m][i] W[o][i] + b[o]), act = relu if
 * relu != 0 -- bit-identical to anerf_mlp_gemm on the same segments.  With w_alpha [k], b_alpha [1] and alpha (all or
 * none) the kernel also writes alpha[m * ld_alpha] = sum_i a[m][i] w_alpha[i] + b_alpha in fp32 from the rows it
 * stages: feature_linear with alpha_linear beside it (core/networks/nerf.py:141-145; anerf_mlp_gemm computes the alpha
 * column as a 257th output in the layer's split arithmetic instead, so alpha agrees to fp32 rounding, not bit for
 * bit).  w_split: anerf_mlp_split_weights(W, 256, k, ld, 0, precision). */
int anerf_mlp_forward_layer(int64_t m, int32_t k, const anerf_seg* a, int32_t n_a, const void* w_split,
                            int32_t precision, const float* bias, int32_t relu, float* y, int64_t ldy,
                            const float* w_alpha, const float* b_alpha, float* alpha, int64_t ld_alpha, void* stream);
/* ABI 19: the persistent kernel as a plain product of any width, one launch per 256 output columns:
 *   c[m][o] = act(sum_i a[m][i] B[o][i] (+ bias[o])), o < n (n % 4 == 0; bias may be NULL),
 * bit-identical to anerf_mlp_gemm with one output segment {c, ldc, n} (no mask, no accumulation).  b_split:
 * anerf_mlp_split_weights(B, n, k, ld, transpose, precision) -- e.g. an input gradient dX = dY W with b_split the
 * transposed split of W, as the training backward's feature gradient [dY_0 | dY_skip] [W_0 ; W_skip,x] (k 512,
 * n = the encoder columns). */
int anerf_mlp_gemm_persistent(int64_t m, int32_t n, int32_t k, const anerf_seg* a, int32_t n_a, const void* b_split,
                              int32_t precision, const float* bias, int32_t relu, float* c, int64_t ldc, void* stream);

/* ---- The tail of a training step (anerf_step.hip; new entries, no struct: ABI 26 still) --------------------------
 * Trainer.compute_loss / optimize (core/trainer.py:319-483) as short fixed launch sequences that never wait for the
 * host.  Every sum has a fixed shape (per workgroup, then one workgroup over the partials in index order, in double):
 * two calls give the same bits; no atomics.  All pointers are device pointers unless said otherwise. */
#define ANERF_LOSS_MSE 0   /* img2mse */
#define ANERF_LOSS_L1 1    /* img2l1 */
#define ANERF_LOSS_HUBER 2 /* F.smooth_l1_loss(beta) */
#define ANERF_REG_NONE 0
#define ANERF_REG_BCE 1    /* acc2bce(acc, fgs, reduction='off'): eps 1e-8, the mean over fgs < 1 */

/* Workspace bytes of anerf_train_loss for n rays (0: refused, see anerf_last_error). */
size_t anerf_train_loss_workspace(int64_t n);
/* Trainer._compute_nerf_loss (core/trainer.py:353-380) of the fine outputs rgb [n][3], acc [n] and, unless both are
 * NULL, the coarse outputs rgb0, acc0, against target [n][3]:  pred = rgb + (1 - acc) bg when use_background (bg =
 * bgs [n][3], or base_bg when bgs is NULL), loss = mean of the loss kind over pred - target (the coarse one times
 * coarse_weight), the regulariser reg_coef * BCE(acc, fgs [n]) per pass (not coarse-weighted).
 * out [8] = rgb_loss, rgb_loss0, reg_loss, reg_loss0, psnr, psnr0, alpha, total:  psnr = -10 ln(mse) / ln 10 of pred
 * whatever the loss kind, alpha = mean(acc), total = the sum of the four losses; entries of an absent pass or
 * regulariser are 0; no ray with fgs < 1: reg_loss is NaN, as torch's mean of nothing.
 * The workspace (8-byte aligned) keeps the sums for anerf_train_loss_backward. */
int anerf_train_loss(const float* rgb, const float* acc, const float* rgb0, const float* acc0, const float* target,
                     const float* bgs, float base_bg, const float* fgs, int64_t n, int32_t loss_kind, float beta,
                     int32_t use_background, float coarse_weight, int32_t reg_kind, float reg_coef, float* out,
                     void* workspace, size_t workspace_bytes, void* stream);
/* Its gradient: g_rgb [n][3], g_acc [n] (g_rgb0, g_acc0 with the coarse pair) = upstream[0] * d total / d input, with
 * the same arguments and the workspace of the forward call; upstream is a device scalar. */
int anerf_train_loss_backward(const float* rgb, const float* acc, const float* rgb0, const float* acc0,
                              const float* target, const float* bgs, float base_bg, const float* fgs, int64_t n,
                              int32_t loss_kind, float beta, int32_t use_background, float coarse_weight,
                              int32_t reg_kind, float reg_coef, const void* workspace, size_t workspace_bytes,
                              const float* upstream, float* g_rgb, float* g_acc, float* g_rgb0, float* g_acc0,
                              void* stream);

/* Workspace bytes of anerf_pose_loss (0: refused). */
size_t anerf_pose_loss_workspace(int64_t n, int32_t n_joints);
/* Trainer._compute_kp_loss (core/trainer.py:382-441).  cur: the per-ray rotations [n][NJ][3][3] when rot6d (the
 * [:3, :2] block is read, six values in row-major order) or the axis-angle bones [n][NJ][3]; anchor [n_poses][NJ][6 | 3]
 * and anchor_kps [n_poses][NJ][3] are gathered at kp_idx [n] (int64; an index outside [0, n_poses) reads nothing and
 * makes the losses NaN); kps [n][NJ][3].
 *   kp_loss   = coef * mean over n (NJ - 1) of sum_c max(d - tol, 0) where d = (anchor - cur)^2 > tol, joint 0 excluded
 *   temp_loss = temp_coef * mean over n NJ of (|2 cur - prev_cur - next_cur|^2 + |2 kps - prev_kps - next_kps|^2)
 *               * temp_val[n], with prev / next (constants, laid out as cur and kps) and temp_val all given or all NULL
 *   MPJPC     = mean |anchor_kps[kp_idx] - kps| / ext_scale (no gradient)
 * out [4] = kp_loss, temp_loss, MPJPC, kp_loss + temp_loss. */
int anerf_pose_loss(const float* cur, int32_t rot6d, const float* anchor, const int64_t* kp_idx, int64_t n,
                    int32_t n_joints, int64_t n_poses, const float* kps, const float* anchor_kps,
                    const float* prev_cur, const float* next_cur, const float* prev_kps, const float* next_kps,
                    const float* temp_val, float tol, float coef, float temp_coef, float ext_scale, float* out,
                    void* workspace, size_t workspace_bytes, void* stream);
/* Its gradient times upstream[0] (a device scalar): g_cur in cur's layout (rot6d: the third column 0) and, with the
 * temporal term, g_kps [n][NJ][3] (otherwise g_kps may be NULL; given, it is zero-filled). */
int anerf_pose_loss_backward(const float* cur, int32_t rot6d, const float* anchor, const int64_t* kp_idx, int64_t n,
                             int32_t n_joints, int64_t n_poses, const float* kps, const float* prev_cur,
                             const float* next_cur, const float* prev_kps, const float* next_kps,
                             const float* temp_val, float tol, float coef, float temp_coef, const float* upstream,
                             float* g_cur, float* g_kps, void* stream);

/* Workspace bytes of anerf_adam_step over tensors of numel[count] elements (HOST array; 0: refused): one double per
 * chunk of 2048 elements of each tensor. */
size_t anerf_adam_step_workspace(const int64_t* numel, int32_t count);
/* torch.optim.Adam's update (betas, eps, weight_decay as L2; no amsgrad, no maximize) of `count` fp32 tensors given
 * as HOST arrays of device pointers (params, grads, exp_avg, exp_avg_sq) and sizes: update number `step` (>= 1) at
 * learning rate lr, in torch's operation order; any count (64 tensors per launch).  Tensors need 4-byte alignment
 * only (a gradient may be a view); 16-byte aligned ones are read as float4.
 * The same pass writes each chunk's sum of squared gradients to workspace[chunk_base ...] (doubles); with norms [2]
 * (device) a last launch sums chunks [0, chunk_base + this call's) in index order and writes get_gradnorm's
 * (core/trainer.py:191-203) total_norm = sqrt(sum) and avg_norm = sqrt(sum / norm_tensors).  Several calls (tensors
 * at different update numbers) share a workspace through chunk_base; the last passes norms. */
int anerf_adam_step(void* const* params, const void* const* grads, void* const* exp_avg, void* const* exp_avg_sq,
                    const int64_t* numel, int32_t count, double lr, double beta1, double beta2, double eps,
                    double weight_decay, int64_t step, int64_t chunk_base, int32_t norm_tensors, float* norms,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- Scoring rendered frames (anerf_eval.hip; new entries, no struct: ABI 26 still) ------------------------------
 * PSNR's squared error and SSIM of F frames of one size H x W where they lie, for evaluate_metric
 * (core/utils/evaluation_helpers.py:257-385) and run_render.py:883-968's scores inside a box.
 * SSIM is Wang et al.'s, per channel: an 11-tap Gaussian window (sigma 1.5, normalised to sum 1) applied separably,
 * K1 = 0.01, K2 = 0.03, C1 = (K1 data_range)^2, C2 = (K2 data_range)^2, mu = E[.], var = E[.^2] - mu^2,
 *   map = ((2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1)) * ((2 cov_xy + C2) / (var_x + var_y + C2)),
 * with moments, map and sums in double (the inputs widen exactly). */
#define ANERF_EVAL_SAME 0  /* zeros outside the rectangle, weights not renormalised (a conv2d with padding 5) */
#define ANERF_EVAL_VALID 1 /* the scored pixels lose 5 per side of the rectangle: windows that lie inside it only */

/* Workspace bytes of anerf_eval_frames: nine doubles per frame and 32 x 16 tile (0: refused, see anerf_last_error). */
size_t anerf_eval_workspace(int32_t n_frames, int32_t H, int32_t W);
/* pred [F][H][W][3] fp32; gt the same, or bytes when gt_uint8 (a byte v is the fp32 that v / 255. rounds to); mask
 * [F][H][W] bytes (nonzero = 1) or NULL (all ones).  rects and boxes are HOST arrays [F][4] of x0, y0, x1, y1 with
 * exclusive upper bounds: a frame's rectangle is what the SSIM filter takes as the image (everything outside it is 0
 * to the filter and is not scored; an empty one is legal and gives zero sums), its box a second, rectangular weight
 * (boxes NULL: all ones).
 *   sums [F][9] (device, double) = { n, sum se, sum ssim } over the scored pixels, over those with the mask set, over
 *   those inside the box: n counts pixels, se = (gt - pred)^2 and ssim are summed over the 3 channels.
 *   map [F][H][W][3] (device, may be NULL): the SSIM map rounded to fp32, 0 at every pixel that is not scored.
 * Each workgroup writes its tile's nine sums to its own workspace slot and a last workgroup per frame adds the
 * frame's slots in tile order: no atomics, the same bits on every run and whatever other frames are in the call.
 * Allocation-free, asynchronous on `stream`, no host read (64 frames per launch).  ANERF_EINVAL, before any launch,
 * for a NULL pred, gt, rects, sums or workspace, a negative size, H or W above 32768, a rectangle or box that is not
 * 0 <= x0 <= x1 <= W, 0 <= y0 <= y1 <= H, an unknown border, data_range <= 0, a workspace not 8-byte aligned;
 * ANERF_EWORKSPACE for a workspace that is too small. */
int anerf_eval_frames(const float* pred, const void* gt, int32_t gt_uint8, const uint8_t* mask, const int32_t* rects,
                      const int32_t* boxes, int32_t n_frames, int32_t H, int32_t W, double data_range, int32_t border,
                      float* map, double* sums, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Pose sequences and the inverse rotation map (anerf_sequence.hip; new entries, no struct: ABI 26 still) -------
 * The bones of run_render.py's render types (lines 484-865) for F output frames from K key poses, in one launch, and
 * matrix -> axis-angle, the inverse of anerf_pose_kinematics' axis-angle branch.  Arithmetic in double, outputs
 * rounded once to float; a thread per output element, no LDS and no atomics, the same bits on every run. */

/* rots [n][9] (row-major 3x3) or [n][6] (rot6d_to_rotmat's parameters, applied first as anerf_pose_kinematics does)
 * -> axisang_out [n][3]: pytorch3d's matrix_to_axis_angle.  The quaternion comes from the best conditioned of the
 * four candidates, is normalised (the input may be orthogonal only to float rounding) and gets a real part >= 0, so
 * the angle lies in [0, pi]; the axis-angle uses sin(half) / angle with the series 0.5 - angle^2 / 48 below 1e-6,
 * as the forward map.  Finite at the identity, at angles of 1e-8 and next to pi (where the sign of the axis is free).
 * Asynchronous on `stream`.  ANERF_EINVAL, before any launch, for another rot_dim, n outside [0, 2^40) or a NULL
 * pointer with n > 0. */
int anerf_rotation_to_axis_angle(const float* rots, int32_t rot_dim, int64_t n, float* axisang_out, void* stream);

#define ANERF_SEQ_LINEAR 0 /* the reference's lerp of axis-angle vectors, a (1 - w) + b w */
#define ANERF_SEQ_SLERP 1  /* per joint: axis-angle -> quaternion -> slerp along the shorter arc -> axis-angle */
#define ANERF_SEQ_ROOT_KEEP 0
#define ANERF_SEQ_ROOT_CONST 1   /* every key's root bone reads as root_const[3] (undo_rot: 1.5708, 0, 0) */
#define ANERF_SEQ_ROOT_COMPOSE 2 /* root = axis-angle of rotate_{x,y,z}(angle_f) R(root): load_pose_rotate */

/* key_bones [K][NJ][3] axis-angle and key_root [K][3] (device) -> bones_out [F][NJ][3], pelvis_out [F][3] (device).
 * A frame's row of frame_keys [F][5] holds its first key, its second key, its base key, its pelvis key and the id of
 * its root-rotation axis (0 x, 1 y, 2 z: skeleton_utils.py's rotate_x / _y / _z); its row of frame_vals [F][2] the
 * weight w of the second key (the double of np.linspace(0, 1, n_step, endpoint=False)) and the root-rotation angle.
 * Both tables are given twice, on the host (checked here: every key in [0, K), the axis id in [0, 2] under
 * ANERF_SEQ_ROOT_COMPOSE, finite values) and on the device (read by the kernel; the caller uploads them once).
 *   bone j of frame f = interp(key first, key second; w)  where joint_mask[j] != 0 (host [NJ]; NULL: every joint),
 *                     = key base                            elsewhere (load_animate's joints),
 *   pelvis of frame f = key_root[pelvis key].
 * ANERF_SEQ_SLERP falls back to lerp-and-normalise of the quaternions when their dot product exceeds 1 - 1e-12
 * (equal keys), and returns the rotation's angle in [0, pi].  The root bone (root_id) follows root_mode.
 * Allocation-free, asynchronous on `stream`.  ANERF_EINVAL, before any launch, for a NULL pointer, K < 1, NJ outside
 * [1, 128], root_id outside [0, NJ), F < 1 or F NJ > 2^31, an unknown interp or root_mode, ANERF_SEQ_ROOT_CONST
 * without root_const (host [3]), or a table entry as above: the kernel never sees an index out of range. */
int anerf_sequence_bones(const float* key_bones, const float* key_root, int32_t n_keys, int32_t n_joints,
                         int32_t root_id, const int32_t* frame_keys_host, const double* frame_vals_host,
                         const int32_t* frame_keys, const double* frame_vals, const uint8_t* joint_mask,
                         int64_t n_frames, int32_t interp, int32_t root_mode, const float* root_const,
                         float* bones_out, float* pelvis_out, void* stream);

/* ---- Scoring refined poses (anerf_posescore.hip; new entries, no struct: ABI 26 still) ---------------------------
 * MPJPE, root-centred MPJPE, least-squares-scaled MPJPE and the Procrustes-aligned PA-MPJPE of F frames of J joints,
 * with the counts PCK and its AUC follow from (core/utils/evaluation_helpers.py:387-612: `procrustes`, the three
 * Criterion* modules, evaluate_pampjpe_from_smpl_params from its line 566 on).  The fit is the reference's
 * procrustes(X = gt, Y = pred): both centred and divided by their Frobenius norms normX, normY, A = X0^T Y0 = U S V^T,
 * T = V U^T, trace = sum(S); with scaling b = trace normX / normY and d = 1 - trace^2, without b = 1 and
 * d = 1 + ssY / ssX - 2 trace normY / normX; Z = b Y T + c, c = muX - b muY T; pa_err = |Z - gt| per joint.
 * Inputs widen exactly and are multiplied by pred_scale / gt_scale into one unit; everything after is double.  The SVD
 * is a one-sided cyclic Jacobi with a fixed sweep count.  T is always orthogonal: where A has rank 2 or 1 (singular
 * values <= 1e-12 of the largest) the missing left singular vectors are completed by cross products to det T = +1
 * (-1 under ANERF_POSE_REFLECT_TRUE), rank 0 gives T = I; the scores do not depend on the completion.  A frame with
 * no scored joint, or whose centred sum of squares on either side is <= 1e-26 of the uncentred one (one joint, all
 * joints equal), has no fit: NaN in pa_mpjpe, d, b, S, T, c, pa_err and aligned, and the totals leave it out. */
#define ANERF_POSE_PRED_F64 1      /* pred is double (default: float) */
#define ANERF_POSE_GT_F64 2        /* gt is double */
#define ANERF_POSE_NO_SCALING 4    /* procrustes(scaling=False) */
#define ANERF_POSE_REFLECT_FALSE 8 /* procrustes(reflection=False): det T = +1 (Kabsch / Umeyama); default 'best' */
#define ANERF_POSE_REFLECT_TRUE 16 /* procrustes(reflection=True): det T = -1 */
#define ANERF_POSE_MAX_JOINTS 128
#define ANERF_POSE_MAX_THRESHOLDS 64
/* A frame's record: n, mpjpe, mpjpe_root, n_mpjpe, pa_mpjpe, d, b, S[3], T[3][3] (row-major), c[3], normX (the
 * extent of gt), normY, s_opt (the least-squares scale of n_mpjpe). */
#define ANERF_POSE_FRAME_COLS 25
/* totals, 8-byte words: [0] frames with a fit, [1] those whose root is valid, [2] those with a finite n_mpjpe,
 * [3..6] the sums of mpjpe, mpjpe_root, n_mpjpe, pa_mpjpe over the frames of [0], [1], [2], [0]; [8 + j] the sum of
 * err at joint j, [136 + j] of pa_err, [264 + j] the count of scored (frame, joint) pairs at joint j (doubles);
 * [392 + k] the pairs with pa_err < thresholds[k], [456 + k] those with err < thresholds[k] (int64). */
#define ANERF_POSE_TOTALS 520

/* Workspace bytes of anerf_pose_scores: the frame records, both error planes and one slot of ANERF_POSE_TOTALS words
 * per 32 frames (0: refused, see anerf_last_error). */
size_t anerf_pose_scores_workspace(int32_t n_frames, int32_t n_joints, int32_t n_thresholds);
/* pred, gt [F][J][3] (device; float, or double under ANERF_POSE_*_F64).  joint_idx: HOST array [n_selected] of the
 * scored joints (NULL: all; the reference's 17-of-24 lists), valid [F][J] bytes (device; NULL: all ones): a pair
 * (frame, joint) is scored where the joint is selected and valid.  root: the joint that mpjpe_root and n_mpjpe
 * subtract from both sides, -1 for none; where it is not valid both are NaN (it need not be selected).  n_mpjpe scales
 * pred by s_opt = <pred, gt> / <pred, pred> over the root-centred scored joints.  thresholds: HOST array.
 *   totals [ANERF_POSE_TOTALS] (device): as above, over the frames with a fit; a frame's means are over its scored
 *     joints.
 *   frames [F][ANERF_POSE_FRAME_COLS], err [F][J], pa_err [F][J] (device, double, each may be NULL: kept in the
 *     workspace): the records and the error planes, 0 at joints that are not scored (err is set in frames without a
 *     fit too).  aligned [F][J][3] (device, float, may be NULL): Z of every joint, rounded once.
 * A wavefront scores a frame, lane l holding joints l and l + 64 in joint order, with one __shfl_xor butterfly per
 * sum; a workgroup per 32 frames adds its slot and a last workgroup the slots in order: no atomics, the same bits
 * on every run, a frame's record the same whatever other frames are in the call.  Allocation-free, asynchronous on
 * `stream`, no host read.  n_frames == 0 returns ANERF_OK without a launch (totals is not written).  ANERF_EINVAL,
 * before any HIP call, for a NULL pred, gt, totals or workspace, n_frames < 0, n_joints outside [1, 128], root
 * outside [-1, J), a joint_idx entry outside [0, J) or repeated, n_selected outside [0, J], more than 64 thresholds
 * (or thresholds NULL with n_thresholds > 0), unknown flag bits or both REFLECT flags, a scale that is not finite, a
 * workspace not 8-byte aligned; ANERF_EWORKSPACE for a workspace that is too small. */
int anerf_pose_scores(const void* pred, const void* gt, int32_t n_frames, int32_t n_joints, const int32_t* joint_idx,
                      int32_t n_selected, const uint8_t* valid, int32_t root, double pred_scale, double gt_scale,
                      int32_t flags, const double* thresholds, int32_t n_thresholds, double* totals, double* frames,
                      double* err, double* pa_err, float* aligned, void* workspace, size_t workspace_bytes,
                      void* stream);

/* ---- Making a dataset: masks, skeleton segments, median backgrounds (anerf_prep.hip; new entries, no struct: ABI 26
 * still) ------------------------------------------------------------------------------------------------------------
 * The pixel-level steps of the reference's loaders (dilate_masks, get_mask, create_kp_mask, draw_skeleton2d, the
 * per-camera median backgrounds) on byte images where they lie.  Every decision is an integer decision, no entry uses
 * atomics, and each gives the same bits on every run.  All three are allocation-free and asynchronous on `stream`,
 * validate before any launch (ANERF_EINVAL with anerf_last_error) and read nothing back. */
#define ANERF_MORPH_DILATE 0 /* maximum over the window */
#define ANERF_MORPH_ERODE 1  /* minimum over the window */
#define ANERF_PREP_MAX_RADIUS 32
#define ANERF_PREP_MAX_DIM 32768
#define ANERF_PREP_MAX_SEGMENTS 128
#define ANERF_PREP_MAX_COORD 8192 /* anerf_draw_segments: H, W and the magnitude of an endpoint's coordinates */
#define ANERF_PREP_MAX_WIDTH 4096
#define ANERF_PREP_MAX_CAMERA_FRAMES (1 << 20) /* anerf_background_median: frames in one camera's list (int32 counters) */

/* src, dst [n_masks][H][W] bytes (device, any values; dst must not be src).  dst = the maximum (ANERF_MORPH_DILATE) or
 * minimum (ANERF_MORPH_ERODE) of src over the square window of half-width `radius` around each pixel; window
 * positions outside the mask are ignored (cv2's default morphology border).  `iterations` applications of a k x k
 * all-ones element, k odd, are one window of radius iterations (k - 1) / 2.  radius 0 copies.
 *   band > 0 (with ANERF_MORPH_DILATE; load_zju.py's get_mask): afterwards dst = 0 wherever
 *     (uint8)(dilate(src, band) - erode(src, band)) == 1.
 *   other != NULL ([n_masks][H][W] bytes; may be dst): afterwards dst = (dst != 0) | (other != 0) as 0 / 1 bytes.
 * One separable pass over an LDS tile with a halo of max(radius, band): a pixel costs O(radius + band).
 * ANERF_EINVAL for a NULL src or dst, dst == src, an unknown op, n_masks < 0, H or W outside [1, 32768], radius or
 * band outside [0, 32], a band with ANERF_MORPH_ERODE, n_masks x tiles (64 x 32 pixels each) >= 2^31. */
int anerf_mask_morph(const uint8_t* src, uint8_t* dst, int64_t n_masks, int32_t H, int32_t W, int32_t op,
                     int32_t radius, int32_t band, const uint8_t* other, void* stream);

/* segs [n_frames][n_segs][4] int32 (device): the endpoints (px, py, qx, qy) of each frame's segments.  Segment b covers
 * the pixel with integer centre c iff the squared distance from c to the closed segment [p, q] is <= (width / 2)^2,
 * decided in int64 with d = q - p, e = c - p, t = e . d:
 *   t <= 0: 4 |c - p|^2 <= width^2;  t >= |d|^2: 4 |c - q|^2 <= width^2;  else 4 cross(d, e)^2 <= width^2 |d|^2.
 * A zero-length segment is a disc.  Where several segments cover a pixel the highest index wins.  A segment with an
 * endpoint coordinate outside [-8192, 8192] is dropped (not clamped).  With H, W <= 8192 every coordinate difference
 * is at most 2^14 in magnitude, so |t|, |d|^2 <= 2^29, |cross| < 2^29, the left sides stay under 2^60 and, with
 * width <= 4096, the right side under 2^53: exact.
 *   mask   [n_frames][H][W] bytes (device, may be NULL): 1 where a segment covers, else 0 (every pixel is written).
 *   frames [n_frames][H][W][3] bytes (device, may be NULL): painted in place, a covered pixel takes colors[b]
 *     (colors [n_segs][3] bytes, device) of the winning segment, every other byte is left as it is.
 * The result does not depend on the schedule (a workgroup per 32 x 16 tile and frame, the frame's segments culled
 * against the tile).  ANERF_EINVAL for neither output, frames without colors, n_frames < 0, n_segs outside [0, 128],
 * segs NULL with n_segs > 0, H or W outside [1, 8192], width outside [1, 4096], n_frames x tiles >= 2^31. */
int anerf_draw_segments(const int32_t* segs, int32_t n_frames, int32_t n_segs, int32_t H, int32_t W, int32_t width,
                        const uint8_t* colors, uint8_t* mask, uint8_t* frames, void* stream);

/* imgs [n_imgs][n_pixels][3] bytes, masks [n_imgs][n_pixels] bytes or NULL (device).  Camera c's frames are
 * order[cam_start[c] .. cam_start[c + 1]) (order [M] and cam_start [n_cams + 1] int32, both given twice: on the host,
 * checked here, and on the device, read by the kernel; the caller uploads them once).  For every camera, pixel and
 * channel: of the listed frames (with masks: those whose mask byte at the pixel is 0) with n taken and their values
 * v ascending, bkgds = floor((v[(n - 1) / 2] + v[n / 2]) / 2), which is np.median(...).astype(np.uint8); n == 0 gives 0.
 *   bkgds [n_cams][n_pixels][3] bytes, counts [n_cams][n_pixels] int32 or NULL: n (device).
 * A thread per (camera, pixel) bisects on the value with int32 counters: a camera lists at most
 * ANERF_PREP_MAX_CAMERA_FRAMES frames.  ANERF_EINVAL for a NULL imgs, bkgds or cam_start, n_imgs outside [0, 2^31),
 * n_pixels outside [1, 2^30], n_cams outside [0, 65535], cam_start[0] != 0 or decreasing, a camera over the limit, order
 * NULL with M > 0, an order entry outside [0, n_imgs): the kernel never sees an index out of range. */
int anerf_background_median(const uint8_t* imgs, const uint8_t* masks, int64_t n_imgs, int64_t n_pixels,
                            const int32_t* order_host, const int32_t* cam_start_host, const int32_t* order,
                            const int32_t* cam_start, int32_t n_cams, uint8_t* bkgds, int32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ANERF_H */

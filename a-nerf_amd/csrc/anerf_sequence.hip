// anerf_sequence.hip — the pose sequences of run_render.py on the device, and the inverse rotation map.
//
// The reference builds the bones of a bullet-time orbit, a pose interpolation, a root rotation, an animation of some
// joints, a retarget clip or a correction clip on the host (run_render.py:484-865: load_correction, load_retarget,
// load_animate, load_pose_rotate, load_interpolate, load_bullettime, load_selected, load_bubble) and chains them one
// frame at a time.  Here one launch writes every output frame's bones and pelvis from K key poses and two small
// per-frame tables, and anerf_pose_kinematics chains them where they lie:
//
//   anerf_sequence_bones          sequence_bones_kernel   a thread per (frame, joint): the frame's two keys, the weight,
//                                                         lerp or slerp, the root mode; the frame's pelvis
//   anerf_rotation_to_axis_angle  rot_to_axisang_kernel   a thread per rotation: 3x3 or 6-D -> axis-angle, the inverse
//                                                         of the axis-angle branch of anerf_pose_kinematics
//                                                         (pytorch3d's matrix_to_axis_angle: matrix -> unit
//                                                         quaternion, real part >= 0 -> axis-angle)
//
// Arithmetic is double, as the chain's; outputs are rounded once to float.  No LDS, no atomics: a thread reads its
// own inputs and writes its own outputs, so two runs give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/anerf.h"

int anerf_internal_fail(int code, const char* msg);  // anerf_render.hip: sets anerf_last_error()

namespace {

constexpr int NTHR = 256;            // threads per workgroup (4 waves of 64)
constexpr int MAX_BLOCKS = 2048;     // the grid's cap: further elements by a grid stride
constexpr int SEQ_MAX_JOINTS = 128;  // anerf_pose_kinematics' limit
constexpr int NT = 5;                // int columns of a frame: first key, second key, base key, pelvis key, axis id
constexpr int NV = 2;                // double columns of a frame: weight, root-rotation angle

struct SeqArgs {
    const float* key_bones;  // [K][NJ][3]
    const float* key_root;   // [K][3]
    const int32_t* ftab;     // [F][NT]
    const double* fval;      // [F][NV]
    float* bones;            // [F][NJ][3]
    float* pelvis;           // [F][3]
    int64_t n_frames;
    int32_t n_keys, nj, root, interp, root_mode;
    float root_const[3];
    uint8_t mask[SEQ_MAX_JOINTS];
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

// axis_angle_to_quaternion (pytorch3d), as the axis-angle branch of anerf_pose_kinematics
__device__ __forceinline__ void axisang_to_quat(const double v[3], double q[4]) {
    const double a = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double half = 0.5 * a;
    const double sho = (a < 1e-6) ? 0.5 - a * a / 48.0 : sin(half) / a;
    q[0] = cos(half);
    q[1] = v[0] * sho;
    q[2] = v[1] * sho;
    q[3] = v[2] * sho;
}

// quaternion_to_matrix (pytorch3d), row-major
__device__ __forceinline__ void quat_to_matrix(const double q[4], double R[9]) {
    const double r = q[0], i = q[1], j = q[2], k = q[3];
    const double two_s = 2.0 / (r * r + i * i + j * j + k * k);
    R[0] = 1.0 - two_s * (j * j + k * k); R[1] = two_s * (i * j - k * r); R[2] = two_s * (i * k + j * r);
    R[3] = two_s * (i * j + k * r); R[4] = 1.0 - two_s * (i * i + k * k); R[5] = two_s * (j * k - i * r);
    R[6] = two_s * (i * k - j * r); R[7] = two_s * (j * k + i * r); R[8] = 1.0 - two_s * (i * i + j * j);
}

// rot6d_to_rotmat (skeleton_utils.py:420-436), as the 6-D branch of anerf_pose_kinematics
__device__ __forceinline__ void rot6d_to_matrix(const float* p, double R[9]) {
    const double a1x = p[0], a1y = p[2], a1z = p[4], a2x = p[1], a2y = p[3], a2z = p[5];
    const double n1 = fmax(sqrt(a1x * a1x + a1y * a1y + a1z * a1z), 1e-12);
    const double b1x = a1x / n1, b1y = a1y / n1, b1z = a1z / n1;
    const double d = b1x * a2x + b1y * a2y + b1z * a2z;
    const double cx = a2x - d * b1x, cy = a2y - d * b1y, cz = a2z - d * b1z;
    const double n2 = fmax(sqrt(cx * cx + cy * cy + cz * cz), 1e-12);
    const double b2x = cx / n2, b2y = cy / n2, b2z = cz / n2;
    const double b3x = b1y * b2z - b1z * b2y, b3y = b1z * b2x - b1x * b2z, b3z = b1x * b2y - b1y * b2x;
    R[0] = b1x; R[1] = b2x; R[2] = b3x;
    R[3] = b1y; R[4] = b2y; R[5] = b3y;
    R[6] = b1z; R[7] = b2z; R[8] = b3z;
}

// matrix_to_quaternion (pytorch3d): of the four candidates the one with the largest |component| it divides by
// (the best conditioned), normalised (the input may be orthogonal only to float rounding), real part >= 0
__device__ __forceinline__ void matrix_to_quat(const double R[9], double q[4]) {
    const double m00 = R[0], m01 = R[1], m02 = R[2], m10 = R[3], m11 = R[4], m12 = R[5];
    const double m20 = R[6], m21 = R[7], m22 = R[8];
    const double s0 = fmax(0.0, 1.0 + m00 + m11 + m22), s1 = fmax(0.0, 1.0 + m00 - m11 - m22);
    const double s2 = fmax(0.0, 1.0 - m00 + m11 - m22), s3 = fmax(0.0, 1.0 - m00 - m11 + m22);
    double c[4];
    double best = s0;
    c[0] = s0; c[1] = m21 - m12; c[2] = m02 - m20; c[3] = m10 - m01;
    if (s1 > best) {
        best = s1;
        c[0] = m21 - m12; c[1] = s1; c[2] = m10 + m01; c[3] = m02 + m20;
    }
    if (s2 > best) {
        best = s2;
        c[0] = m02 - m20; c[1] = m10 + m01; c[2] = s2; c[3] = m12 + m21;
    }
    if (s3 > best) {
        best = s3;
        c[0] = m10 - m01; c[1] = m20 + m02; c[2] = m21 + m12; c[3] = s3;
    }
    const double den = 2.0 * fmax(sqrt(best), 0.1);
    double n2 = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        q[e] = c[e] / den;
        n2 += q[e] * q[e];
    }
    const double inv = (n2 > 0.0) ? 1.0 / sqrt(n2) : 1.0;
    const double sgn = (q[0] < 0.0) ? -inv : inv;
#pragma unroll
    for (int e = 0; e < 4; ++e) q[e] *= sgn;
}

// quaternion_to_axis_angle (pytorch3d) of a unit quaternion with q[0] >= 0: the angle lies in [0, pi]
__device__ __forceinline__ void quat_to_axisang(const double q[4], double v[3]) {
    const double n = sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double half = atan2(n, q[0]);
    const double a = 2.0 * half;
    const double sho = (a < 1e-6) ? 0.5 - a * a / 48.0 : sin(half) / a;
    v[0] = q[1] / sho;
    v[1] = q[2] / sho;
    v[2] = q[3] / sho;
}

// rotate_x / rotate_y / rotate_z (skeleton_utils.py:21-42; rotate_y carries the reference's sign) times R
__device__ __forceinline__ void rotate_axis(int axis, double angle, const double R[9], double out[9]) {
    const double c = cos(angle), s = sin(angle);
    double A[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    if (axis == 0) {
        A[4] = c; A[5] = -s; A[7] = s; A[8] = c;
    } else if (axis == 1) {
        A[0] = c; A[2] = -s; A[6] = s; A[8] = c;
    } else {
        A[0] = c; A[1] = -s; A[3] = s; A[4] = c;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int cc = 0; cc < 3; ++cc)
            out[3 * r + cc] = A[3 * r] * R[cc] + A[3 * r + 1] * R[3 + cc] + A[3 * r + 2] * R[6 + cc];
}

__device__ __forceinline__ void key_bone(const SeqArgs& a, int k, int j, double v[3]) {
    if (j == a.root && a.root_mode == ANERF_SEQ_ROOT_CONST) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = a.root_const[c];
        return;
    }
    const float* p = a.key_bones + ((size_t)k * a.nj + j) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = p[c];
}

__global__ __launch_bounds__(NTHR) void sequence_bones_kernel(SeqArgs a) {
    const int64_t total = a.n_frames * a.nj;
    for (int64_t t = (int64_t)blockIdx.x * NTHR + threadIdx.x; t < total; t += (int64_t)gridDim.x * NTHR) {
        const int64_t f = t / a.nj;
        const int j = (int)(t - f * a.nj);
        const int32_t* ft = a.ftab + f * NT;
        const int k0 = ft[0], k1 = ft[1], kb = ft[2], kp = ft[3], axis = ft[4];
        const double w = a.fval[f * NV], angle = a.fval[f * NV + 1];
        float* o = a.bones + t * 3;
        // (the host checked its copy of the tables; a key outside [0, K) here is never read through)
        const unsigned K = (unsigned)a.n_keys;
        if ((unsigned)k0 >= K || (unsigned)k1 >= K || (unsigned)kb >= K || (unsigned)kp >= K) {
            o[0] = o[1] = o[2] = __builtin_nanf("");
            if (j == 0) a.pelvis[f * 3] = a.pelvis[f * 3 + 1] = a.pelvis[f * 3 + 2] = __builtin_nanf("");
            continue;
        }
        double v[3];
        if (!a.mask[j]) {
            key_bone(a, kb, j, v);
        } else {
            double x[3], y[3];
            key_bone(a, k0, j, x);
            key_bone(a, k1, j, y);
            if (a.interp == ANERF_SEQ_LINEAR) {
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = x[c] * (1.0 - w) + y[c] * w;
            } else {
                double p[4], q[4], r[4];
                axisang_to_quat(x, p);
                axisang_to_quat(y, q);
                double dot = p[0] * q[0] + p[1] * q[1] + p[2] * q[2] + p[3] * q[3];
                if (dot < 0.0) {  // the shorter arc
                    dot = -dot;
#pragma unroll
                    for (int e = 0; e < 4; ++e) q[e] = -q[e];
                }
                double wa = 1.0 - w, wb = w;
                if (dot <= 1.0 - 1e-12) {
                    const double th = acos(dot), st = sin(th);
                    wa = sin((1.0 - w) * th) / st;
                    wb = sin(w * th) / st;
                }
                double n2 = 0.0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    r[e] = wa * p[e] + wb * q[e];
                    n2 += r[e] * r[e];
                }
                const double inv = (n2 > 0.0) ? 1.0 / sqrt(n2) : 1.0;
                const double sgn = (r[0] < 0.0) ? -inv : inv;
#pragma unroll
                for (int e = 0; e < 4; ++e) r[e] *= sgn;
                quat_to_axisang(r, v);
            }
        }
        if (j == a.root && a.root_mode == ANERF_SEQ_ROOT_COMPOSE) {
            double q[4], R[9], M[9];
            axisang_to_quat(v, q);
            quat_to_matrix(q, R);
            rotate_axis(axis, angle, R, M);
            matrix_to_quat(M, q);
            quat_to_axisang(q, v);
        }
        o[0] = (float)v[0];
        o[1] = (float)v[1];
        o[2] = (float)v[2];
        if (j == 0) {
            const float* pr = a.key_root + (size_t)kp * 3;
            a.pelvis[f * 3] = pr[0];
            a.pelvis[f * 3 + 1] = pr[1];
            a.pelvis[f * 3 + 2] = pr[2];
        }
    }
}

__global__ __launch_bounds__(NTHR) void rot_to_axisang_kernel(const float* __restrict__ rots, int rot_dim, int64_t n,
                                                              float* __restrict__ out) {
    for (int64_t t = (int64_t)blockIdx.x * NTHR + threadIdx.x; t < n; t += (int64_t)gridDim.x * NTHR) {
        const float* p = rots + t * rot_dim;
        double R[9], q[4], v[3];
        if (rot_dim == 6) {
            rot6d_to_matrix(p, R);
        } else {
#pragma unroll
            for (int e = 0; e < 9; ++e) R[e] = p[e];
        }
        matrix_to_quat(R, q);
        quat_to_axisang(q, v);
        out[t * 3] = (float)v[0];
        out[t * 3 + 1] = (float)v[1];
        out[t * 3 + 2] = (float)v[2];
    }
}

inline unsigned blocks_for(int64_t n) {
    const int64_t b = (n + NTHR - 1) / NTHR;
    return (unsigned)(b < MAX_BLOCKS ? b : MAX_BLOCKS);
}

}  // namespace

extern "C" {

int anerf_rotation_to_axis_angle(const float* rots, int32_t rot_dim, int64_t n, float* axisang_out, void* stream) {
    const char* fn = "anerf_rotation_to_axis_angle";
    if (rot_dim != 9 && rot_dim != 6) return fail(fn, "rot_dim must be 9 (row-major 3x3) or 6");
    if (n < 0 || n >= ((int64_t)1 << 40)) return fail(fn, "n must be in [0, 2^40)");
    if (n == 0) return ANERF_OK;
    if (!rots || !axisang_out) return fail(fn, "rots and axisang_out must not be NULL");
    hipLaunchKernelGGL(rot_to_axisang_kernel, dim3(blocks_for(n)), dim3(NTHR), 0, (hipStream_t)stream, rots,
                       (int)rot_dim, n, axisang_out);
    return launched(fn);
}

int anerf_sequence_bones(const float* key_bones, const float* key_root, int32_t n_keys, int32_t n_joints,
                         int32_t root_id, const int32_t* frame_keys_host, const double* frame_vals_host,
                         const int32_t* frame_keys, const double* frame_vals, const uint8_t* joint_mask,
                         int64_t n_frames, int32_t interp, int32_t root_mode, const float* root_const,
                         float* bones_out, float* pelvis_out, void* stream) {
    const char* fn = "anerf_sequence_bones";
    if (!key_bones || !key_root || !frame_keys_host || !frame_vals_host || !frame_keys || !frame_vals || !bones_out ||
        !pelvis_out)
        return fail(fn, "key_bones, key_root, the frame tables (host and device), bones_out and pelvis_out must not "
                        "be NULL");
    if (n_keys < 1) return fail(fn, "n_keys must be >= 1");
    if (n_joints < 1 || n_joints > SEQ_MAX_JOINTS) return fail(fn, "n_joints must be in [1, 128]");
    if (root_id < 0 || root_id >= n_joints) return fail(fn, "root_id must be in [0, n_joints)");
    if (n_frames < 1 || n_frames > ((int64_t)1 << 31) / n_joints)
        return fail(fn, "n_frames must be >= 1 and n_frames n_joints <= 2^31");
    if (interp != ANERF_SEQ_LINEAR && interp != ANERF_SEQ_SLERP)
        return fail(fn, "unknown interp (ANERF_SEQ_LINEAR or ANERF_SEQ_SLERP)");
    if (root_mode != ANERF_SEQ_ROOT_KEEP && root_mode != ANERF_SEQ_ROOT_CONST && root_mode != ANERF_SEQ_ROOT_COMPOSE)
        return fail(fn, "unknown root_mode (ANERF_SEQ_ROOT_KEEP, _CONST or _COMPOSE)");
    if (root_mode == ANERF_SEQ_ROOT_CONST && !root_const) return fail(fn, "ANERF_SEQ_ROOT_CONST needs root_const");
    for (int64_t f = 0; f < n_frames; ++f) {
        const int32_t* ft = frame_keys_host + f * NT;
        for (int c = 0; c < 4; ++c)
            if (ft[c] < 0 || ft[c] >= n_keys) {
                char msg[160];
                snprintf(msg, sizeof msg, "frame %lld: key column %d = %d is outside [0, n_keys = %d)", (long long)f, c,
                         ft[c], n_keys);
                return fail(fn, msg);
            }
        if (root_mode == ANERF_SEQ_ROOT_COMPOSE && (ft[4] < 0 || ft[4] > 2)) {
            char msg[160];
            snprintf(msg, sizeof msg, "frame %lld: axis id %d is not 0 (x), 1 (y) or 2 (z)", (long long)f, ft[4]);
            return fail(fn, msg);
        }
        if (!std::isfinite(frame_vals_host[f * NV]) || !std::isfinite(frame_vals_host[f * NV + 1])) {
            char msg[160];
            snprintf(msg, sizeof msg, "frame %lld: the weight and the angle must be finite", (long long)f);
            return fail(fn, msg);
        }
    }
    SeqArgs a;
    a.key_bones = key_bones;
    a.key_root = key_root;
    a.ftab = frame_keys;
    a.fval = frame_vals;
    a.bones = bones_out;
    a.pelvis = pelvis_out;
    a.n_frames = n_frames;
    a.n_keys = n_keys;
    a.nj = n_joints;
    a.root = root_id;
    a.interp = interp;
    a.root_mode = root_mode;
    for (int c = 0; c < 3; ++c) a.root_const[c] = (root_mode == ANERF_SEQ_ROOT_CONST) ? root_const[c] : 0.f;
    for (int j = 0; j < SEQ_MAX_JOINTS; ++j) a.mask[j] = (j < n_joints) ? (joint_mask ? joint_mask[j] != 0 : 1) : 0;
    hipLaunchKernelGGL(sequence_bones_kernel, dim3(blocks_for(n_frames * n_joints)), dim3(NTHR), 0, (hipStream_t)stream,
                       a);
    return launched(fn);
}

}  // extern "C"

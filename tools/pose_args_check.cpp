// Stand-alone check of anerf_pose_scores' argument validation, for a host sanitizer build: every call below is
// refused (or, with no frame, accepted) before any HIP call, so the program runs on a machine without a GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -o pose_args_check tools/pose_args_check.cpp a-nerf_amd/csrc/anerf_posescore.hip && ./pose_args_check
//
// Nothing sanitized is loaded into Python: the unit under test is compiled into this program.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/anerf.h"

static std::string g_last;

// anerf_render.hip's in the library: here the message is kept for the checks below
int anerf_internal_fail(int code, const char* msg) {
    g_last = msg;
    return code;
}

static int g_failed = 0;

static void expect(const char* what, int rc, int want, const char* word) {
    const bool ok = rc == want && (want == ANERF_OK || (g_last.rfind("anerf_pose_scores", 0) == 0 &&
                                                       g_last.find(word) != std::string::npos));
    if (!ok) {
        ++g_failed;
        std::printf("FAILED %s: rc %d (want %d), message '%s' (want '%s')\n", what, rc, want, g_last.c_str(), word);
    }
}

int main() {
    const int F = 3, J = 24;
    std::vector<double> buf((size_t)F * J * 3), totals(ANERF_POSE_TOTALS), th(64);
    const size_t need = anerf_pose_scores_workspace(F, J, 31);
    std::vector<double> ws(need / 8 + 1);
    for (int k = 0; k < 64; ++k) th[k] = 5.0 * k;
    struct Call {
        const void* pred;
        const void* gt;
        int F, J;
        std::vector<int32_t> idx;
        int n_sel;
        int root;
        double scale;
        int flags;
        const double* th;
        int nt;
        double* totals;
        void* ws;
        size_t bytes;
    };
    const Call ok{buf.data(), buf.data(), F, J, {}, -1, 0, 1.0, 0, th.data(), 31, totals.data(), ws.data(), need};
    auto run = [&](const Call& c) {
        g_last.clear();
        const int n_sel = c.n_sel >= 0 ? c.n_sel : (int)c.idx.size();
        return anerf_pose_scores(c.pred, c.gt, c.F, c.J, c.idx.empty() ? nullptr : c.idx.data(), n_sel, nullptr, c.root,
                                 c.scale, 1.0, c.flags, c.th, c.nt, c.totals, nullptr, nullptr, nullptr, nullptr, c.ws,
                                 c.bytes, nullptr);
    };
    Call c = ok;
    c.pred = nullptr;
    expect("null pred", run(c), ANERF_EINVAL, "pred");
    c = ok, c.gt = nullptr;
    expect("null gt", run(c), ANERF_EINVAL, "gt");
    c = ok, c.totals = nullptr;
    expect("null totals", run(c), ANERF_EINVAL, "totals");
    c = ok, c.F = -1;
    expect("n_frames < 0", run(c), ANERF_EINVAL, "n_frames");
    c = ok, c.J = 0;
    expect("n_joints 0", run(c), ANERF_EINVAL, "n_joints");
    c = ok, c.J = 129;
    expect("n_joints 129", run(c), ANERF_EINVAL, "n_joints");
    c = ok, c.root = J;
    expect("root J", run(c), ANERF_EINVAL, "root");
    c = ok, c.root = -2;
    expect("root -2", run(c), ANERF_EINVAL, "root");
    c = ok, c.idx = {0, J};
    expect("joint_idx out of range", run(c), ANERF_EINVAL, "joint_idx[1]");
    c = ok, c.idx = {5, -1};
    expect("joint_idx negative", run(c), ANERF_EINVAL, "joint_idx[1]");
    c = ok, c.idx = {3, 5, 3};
    expect("joint_idx repeated", run(c), ANERF_EINVAL, "repeated");
    c = ok, c.idx = {1}, c.n_sel = J + 1;
    expect("n_selected", run(c), ANERF_EINVAL, "n_selected");
    c = ok, c.nt = 65;
    expect("65 thresholds", run(c), ANERF_EINVAL, "n_thresholds");
    c = ok, c.th = nullptr;
    expect("null thresholds", run(c), ANERF_EINVAL, "thresholds");
    c = ok, c.flags = 32;
    expect("unknown flag", run(c), ANERF_EINVAL, "unknown flag");
    c = ok, c.flags = ANERF_POSE_REFLECT_FALSE | ANERF_POSE_REFLECT_TRUE;
    expect("both reflect flags", run(c), ANERF_EINVAL, "exclude");
    c = ok, c.scale = 1.0 / 0.0 - 1.0 / 0.0;
    expect("NaN scale", run(c), ANERF_EINVAL, "finite");
    c = ok, c.ws = nullptr;
    expect("null workspace", run(c), ANERF_EINVAL, "workspace");
    c = ok, c.ws = (char*)ws.data() + 4;
    expect("misaligned workspace", run(c), ANERF_EINVAL, "aligned");
    c = ok, c.bytes = need - 8;
    expect("small workspace", run(c), ANERF_EWORKSPACE, "too small");
    c = ok, c.F = 0;
    expect("no frame", run(c), ANERF_OK, "");
    c = ok, c.F = 0, c.idx = std::vector<int32_t>(J);
    for (int j = 0; j < J; ++j) c.idx[j] = J - 1 - j;  // every joint once, the last slot of the mask included
    expect("no frame, all joints listed", run(c), ANERF_OK, "");
    c = ok, c.F = 0, c.J = 128, c.idx = {127, 64, 63, 0};
    expect("no frame, 128 joints", run(c), ANERF_OK, "");
    if (anerf_pose_scores_workspace(-1, J, 0) != 0 || anerf_pose_scores_workspace(1, 129, 0) != 0 ||
        anerf_pose_scores_workspace(1, J, 65) != 0 || anerf_pose_scores_workspace(0, 1, 0) < 8) {
        ++g_failed;
        std::printf("FAILED anerf_pose_scores_workspace's refusals\n");
    }
    std::printf(g_failed ? "%d check(s) failed\n" : "pose_args_check ok\n", g_failed);
    return g_failed != 0;
}

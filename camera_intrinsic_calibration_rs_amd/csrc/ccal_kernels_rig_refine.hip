// Board poses of a whole rig under fixed intrinsics AND extrinsics (ccal_refine_rig_poses_batch): for every frame slot the pose
// T_0_b of the board in the rig frame that minimises
//     sum over the slot's cameras c, corners i of  rho(| project_c(theta_c, T_c_0 o T_0_b X_i) - uv_i |^2)
// with the Huber loss of the joint solve - the OtherCamReprojectionFactor of the reference (factors.rs:179-228) over rvec_0_b |
// tvec_0_b alone.  A slot seen by several cameras has ONE pose, fitted to all of them at once.
// n_slots independent 6-unknown problems in ONE launch, one wavefront per slot, four per workgroup, the whole Levenberg-Marquardt
// solve of a slot inside the launch - the shape, the rule and the shared pieces of k_pose_refine (ccal_refine.hpp).  What is new:
//   a slot owns the SEGMENTS [seg_off[s], seg_off[s + 1]); segment j is one camera's observation of the slot: camera seg_cam[j],
//   corners [pt_off[j], pt_off[j + 1]).  A pass at a pose loops over the segments; per segment
//     - the frame constants of T_c_0 o T_0_b (frame_setup<true> with that camera's extrinsic, every lane the same values),
//     - a wave-uniform switch on the camera's model, load_theta from the argument struct (scalar loads: the parameters of up to
//       CCAL_MAX_CAMS cameras travel in the kernel arguments, no LDS, no barrier),
//     - refine_corners<MODEL, true>: the lanes stride the segment, lane-private f64 sums that carry over from segment to segment,
//   and ONE butterfly after the last segment.  The order of summation is fixed by the slot's own segments and counts: a slot's
//   result does not depend on the batch around it.  No atomics, no LDS.
// A segment shorter than 64 corners leaves lanes idle in its pass; two short segments are NOT packed into one pass (the lanes of a
// pass would then run two model bodies one after the other under exec masks - DESIGN.md).
#include <string>

#include "ccal_refine.hpp"

namespace ccal {

struct RigRefineArgs {
    double th[CCAL_MAX_CAMS][CCAL_PMAX];    // every camera's parameters in the kernels' canonical order
    double extr[CCAL_MAX_CAMS][6];          // rvec | tvec of T_c_0
    int32_t model[CCAL_MAX_CAMS];
    ModelRt rt;
    const int64_t* seg_off;             // [n_slots + 1]
    const int64_t* pt_off;              // [n_seg + 1]
    const int32_t* seg_cam;             // [n_seg]
    const double* xyz; const double* uv;     // [.][3], [.][2] pixels
    double* poses;                      // [n_slots][6] in: start, out: result
    int32_t* status; int32_t* iters; int32_t* n_used;
    double* cost0; double* cost;        // [n_slots]
    double* err;                        // [n_points] pixel error at the result, or nullptr
    RefineRule rule;                    // n_prob: the number of slots
};

// one segment's corners through its camera's model
template <int MODEL>
__device__ __forceinline__ void rig_segment(const double* th_g, const ModelRt& rt, const double* fc, const double* xyz, const double* uv,
                                            double* err, const int n, const int lane, const double delta, double* H, double* g,
                                            double& cost, double& obj) {
    double th[th_len<MODEL>()];
    load_theta<MODEL, false>(th_g, rt, th);
    refine_corners<MODEL, true>(th, fc, xyz, uv, err, n, lane, delta, H, g, cost, obj);
}

__global__ __launch_bounds__(256) void k_rig_pose_refine(const RigRefineArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int o = blockIdx.x * WAVES_PER_BLOCK + wave;
    if (o >= a.rule.n_prob) return;
    const int64_t s0 = a.seg_off[o], s1 = a.seg_off[o + 1];

    double pose[6];
    bool start_ok = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) { pose[i] = a.poses[(int64_t)o * 6 + i]; start_ok = start_ok && refine_finite(pose[i]); }
    int cnt = 0;
    for (int64_t j = s0; j < s1; ++j) {
        const int64_t p0 = a.pt_off[j];
        const int n = (int)(a.pt_off[j + 1] - p0);
        for (int c = lane; c < n; c += 64) cnt += refine_point_valid(a.xyz + 3 * p0, a.uv + 2 * p0, c) ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (!start_ok || cnt < (a.rule.min_points > 3 ? a.rule.min_points : 3)) {      // no result: the pose stays as the caller gave it
        if (a.err && s1 > s0) {
            const int64_t p0 = a.pt_off[s0], p1 = a.pt_off[s1];        // a slot's segments, and so its points, are contiguous
            for (int64_t c = p0 + lane; c < p1; c += 64) a.err[c] = __builtin_nan("");
        }
        if (lane == 0) {
            a.status[o] = CCAL_NO_RESULT; a.iters[o] = 0; a.n_used[o] = 0; a.cost0[o] = 0.0; a.cost[o] = 0.0;
        }
        return;
    }

    // one pass over all the slot's segments at the pose p: the totals on all lanes
    const double delta = a.rule.delta;
    auto pass = [&](const double* p, const bool with_err, double* H, double* g, double& rep, double& obj) {
        refine_zero(H, g, rep, obj);
        for (int64_t j = s0; j < s1; ++j) {
            const int64_t p0 = a.pt_off[j];
            const int n = (int)(a.pt_off[j + 1] - p0);
            if (n == 0) continue;
            const int cam = a.seg_cam[j];
            const double* xyz = a.xyz + 3 * p0;
            const double* uv = a.uv + 2 * p0;
            double* err = with_err ? a.err + p0 : nullptr;
            double fc[FC_SIZE];
            frame_setup<true>(p, a.extr[cam], fc);
            switch (a.model[cam]) {
                case kUCM: rig_segment<kUCM>(a.th[cam], a.rt, fc, xyz, uv, err, n, lane, delta, H, g, rep, obj); break;
                case kEUCM: rig_segment<kEUCM>(a.th[cam], a.rt, fc, xyz, uv, err, n, lane, delta, H, g, rep, obj); break;
                case kKB4: rig_segment<kKB4>(a.th[cam], a.rt, fc, xyz, uv, err, n, lane, delta, H, g, rep, obj); break;
                default: rig_segment<kOCV5>(a.th[cam], a.rt, fc, xyz, uv, err, n, lane, delta, H, g, rep, obj); break;
            }
        }
        refine_reduce(H, g, rep, obj);
    };
    int iter;
    double cost0, cost;
    const int status = refine_lm(a.rule, a.err != nullptr, pass, pose, iter, cost0, cost);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) a.poses[(int64_t)o * 6 + i] = pose[i];
        a.status[o] = status; a.iters[o] = iter; a.n_used[o] = cnt;
        a.cost0[o] = cost0; a.cost[o] = cost;
    }
}

}  // namespace ccal

using namespace ccal;

namespace {

int fail(ccal_ctx* ctx, int code, const char* msg) { note_error(ctx, msg); return code; }
int hip_fail(ccal_ctx* ctx, const char* where, hipError_t e) {
    try { ctx->err = std::string(where) + ": " + hipGetErrorString(e); } catch (...) { }
    return CCAL_ERR_HIP;
}

}  // namespace

extern "C" {

int ccal_refine_rig_poses_batch(ccal_ctx* ctx, int n_cams, const int32_t* model, const double* params, const double* extr,
                                double huber_delta, int n_slots, const int64_t* seg_offsets, const int32_t* seg_cam,
                                const int64_t* pt_offsets, const double* xyz, const double* uv, int min_points,
                                const ccal_solver_opts* opts, double* poses_io, int32_t* status_out, int32_t* iters_out,
                                int32_t* n_used_out, double* cost0_out, double* cost_out, double* err_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    if (n_cams < 1 || n_cams > CCAL_MAX_CAMS) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_rig_poses_batch: n_cams outside 1 .. CCAL_MAX_CAMS");
    if (!model || !params || !extr) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_rig_poses_batch: NULL argument");
    for (int c = 0; c < n_cams; ++c)
        if (model[c] != CCAL_MODEL_EUCMT && (model[c] < 0 || model[c] >= kNumModels))
            return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_rig_poses_batch: unknown camera model");
    for (int c = 0; c < n_cams; ++c)
        if (model[c] == CCAL_MODEL_EUCMT)
            return fail(ctx, CCAL_ERR_UNSUPPORTED, "ccal_refine_rig_poses_batch: EUCMT is a parameter container in this build (its projection is only in the absent camera-intrinsic-model crate)");
    if (n_slots < 0) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_rig_poses_batch: n_slots < 0");
    if (n_slots == 0) return CCAL_OK;
    if (!seg_offsets || !poses_io || !status_out) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_rig_poses_batch: NULL argument");
    if (seg_offsets[0] != 0) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_rig_poses_batch: seg_offsets[0] != 0");
    for (int i = 0; i < n_slots; ++i)
        if (seg_offsets[i + 1] < seg_offsets[i]) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_rig_poses_batch: seg_offsets must not decrease");
    const size_t n_seg = (size_t)seg_offsets[n_slots], ns = (size_t)n_slots;
    if (n_seg && (!seg_cam || !pt_offsets)) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_rig_poses_batch: NULL argument");
    if (n_seg && pt_offsets[0] != 0) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_rig_poses_batch: pt_offsets[0] != 0");
    for (size_t j = 0; j < n_seg; ++j) {
        if (pt_offsets[j + 1] < pt_offsets[j]) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_rig_poses_batch: pt_offsets must not decrease");
        if (seg_cam[j] < 0 || seg_cam[j] >= n_cams) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_rig_poses_batch: seg_cam out of range");
    }
    for (int i = 0; i < n_slots && n_seg; ++i)
        if (pt_offsets[seg_offsets[i + 1]] - pt_offsets[seg_offsets[i]] > (1 << 24))
            return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_rig_poses_batch: at most 2^24 points in a slot");
    const size_t n_tot = n_seg ? (size_t)pt_offsets[n_seg] : 0;
    if (n_tot && (!xyz || !uv)) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_rig_poses_batch: NULL argument");
    ccal_solver_opts o;
    if (opts) o = *opts; else ccal_set_defaults(&o);
    CCAL_API_TRY
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, "hipSetDevice", e);
    // one block: segment offsets | point offsets | segment cameras | points | image points | poses, cost0, cost | errors |
    // status, iterations, counts
    const size_t b_sof = refine_up256((ns + 1) * 8), b_pof = refine_up256((n_seg + 1) * 8), b_cam = refine_up256((n_seg + 1) * 4);
    const size_t b_xyz = refine_up256((n_tot + 1) * 24), b_uv = refine_up256((n_tot + 1) * 16), b_res = refine_up256(ns * 8 * 8);
    const size_t b_err = err_out ? refine_up256((n_tot + 1) * 8) : 0, b_int = refine_up256(ns * 3 * 4);
    char* d = nullptr;
    e = ctx_dev_alloc(ctx, (void**)&d, b_sof + b_pof + b_cam + b_xyz + b_uv + b_res + b_err + b_int);
    if (e != hipSuccess) return hip_fail(ctx, "ccal_refine_rig_poses_batch: allocation", e);
    struct Guard { ccal_ctx* c; char* p; ~Guard() { (void)hipStreamSynchronize(c->stream); ctx_release(c, p, false); } } guard{ ctx, d };
    RigRefineArgs a = {};
    for (int c = 0; c < n_cams; ++c) {
        const double* pc = params + (size_t)c * CCAL_PMAX;
        for (int i = 0; i < model_np(model[c]); ++i) a.th[c][i] = pc[(model[c] == kOCV5 && i >= 4) ? 4 + ctx->conv.ocv5_order[i - 4] : i];
        for (int i = 0; i < 6; ++i) a.extr[c][i] = extr[(size_t)c * 6 + i];
        a.model[c] = model[c];
    }
    a.rt = model_rt(ctx);
    a.rt.ocv5_perm = kOcv5IdentityPerm;
    int64_t* d_sof = (int64_t*)d;
    int64_t* d_pof = (int64_t*)(d + b_sof);
    int32_t* d_cam = (int32_t*)(d + b_sof + b_pof);
    char* dd = d + b_sof + b_pof + b_cam;            // the blocks of doubles
    double* d_xyz = (double*)dd;
    double* d_uv = (double*)(dd + b_xyz);
    double* d_po = (double*)(dd + b_xyz + b_uv);
    double* d_err = err_out ? (double*)(dd + b_xyz + b_uv + b_res) : nullptr;
    int32_t* d_int = (int32_t*)(dd + b_xyz + b_uv + b_res + b_err);
    a.seg_off = d_sof; a.pt_off = d_pof; a.seg_cam = d_cam; a.xyz = d_xyz; a.uv = d_uv;
    a.poses = d_po; a.cost0 = d_po + ns * 6; a.cost = d_po + ns * 7; a.err = d_err;
    a.status = d_int; a.iters = d_int + ns; a.n_used = d_int + 2 * ns;
    a.rule = refine_rule(huber_delta, o, n_slots, min_points);
    hipStream_t s = ctx->stream;
    e = test_poison_f64(ctx, d_xyz, b_xyz + b_uv + b_res + b_err, false, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_sof, seg_offsets, (ns + 1) * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && n_seg) e = hipMemcpyAsync(d_pof, pt_offsets, (n_seg + 1) * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && n_seg) e = hipMemcpyAsync(d_cam, seg_cam, n_seg * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && n_tot) e = hipMemcpyAsync(d_xyz, xyz, n_tot * 24, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && n_tot) e = hipMemcpyAsync(d_uv, uv, n_tot * 16, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_po, poses_io, ns * 6 * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_rig_pose_refine, dim3((n_slots + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK), dim3(256), 0, s, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(poses_io, d_po, ns * 6 * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(status_out, a.status, ns * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && iters_out) e = hipMemcpyAsync(iters_out, a.iters, ns * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && n_used_out) e = hipMemcpyAsync(n_used_out, a.n_used, ns * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && cost0_out) e = hipMemcpyAsync(cost0_out, a.cost0, ns * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && cost_out) e = hipMemcpyAsync(cost_out, a.cost, ns * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && err_out && n_tot) e = hipMemcpyAsync(err_out, d_err, n_tot * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(ctx, "ccal_refine_rig_poses_batch", e);
    return CCAL_OK;
    CCAL_API_CATCH(ctx)
}

}  // extern "C"

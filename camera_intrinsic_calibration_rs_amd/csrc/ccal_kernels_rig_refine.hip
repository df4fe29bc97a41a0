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
#include <algorithm>
#include "ccal_call.hpp"
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
    RefineIO io;                        // a problem: a slot
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
    if (o >= a.io.rule.n_prob) return;
    const int64_t s0 = a.seg_off[o], s1 = a.seg_off[o + 1];

    double pose[6];
    bool start_ok = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) { pose[i] = a.io.poses[(int64_t)o * 6 + i]; start_ok = start_ok && refine_finite(pose[i]); }
    int cnt = 0;
    for (int64_t j = s0; j < s1; ++j) {
        const int64_t p0 = a.pt_off[j];
        const int n = (int)(a.pt_off[j + 1] - p0);
        for (int c = lane; c < n; c += 64) cnt += refine_point_valid(a.io.xyz + 3 * p0, a.io.uv + 2 * p0, c) ? 1 : 0;
    }
    refine_count(cnt);
    if (!start_ok || cnt < refine_min_points(a.io)) {
        if (a.io.err && s1 > s0) {
            const int64_t p0 = a.pt_off[s0], p1 = a.pt_off[s1];        // a slot's segments, and so its points, are contiguous
            for (int64_t c = p0 + lane; c < p1; c += 64) a.io.err[c] = __builtin_nan("");
        }
        refine_store_none(a.io, o, lane);
        return;
    }

    // one pass over all the slot's segments at the pose p: the totals on all lanes
    const double delta = a.io.rule.delta;
    auto pass = [&](const double* p, const bool with_err, double* H, double* g, double& rep, double& obj) {
        refine_zero(H, g, rep, obj);
        for (int64_t j = s0; j < s1; ++j) {
            const int64_t p0 = a.pt_off[j];
            const int n = (int)(a.pt_off[j + 1] - p0);
            if (n == 0) continue;
            const int cam = a.seg_cam[j];
            const double* xyz = a.io.xyz + 3 * p0;
            const double* uv = a.io.uv + 2 * p0;
            double* err = with_err ? a.io.err + p0 : nullptr;
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
    const int status = refine_lm(a.io.rule, a.io.err != nullptr, pass, pose, iter, cost0, cost);
    refine_store(a.io, o, lane, pose, status, iter, cnt, cost0, cost);
}

}  // namespace ccal

using namespace ccal;

extern "C" {

int ccal_refine_rig_poses_batch(ccal_ctx* ctx, int n_cams, const int32_t* model, const double* params, const double* extr,
                                double huber_delta, int n_slots, const int64_t* seg_offsets, const int32_t* seg_cam,
                                const int64_t* pt_offsets, const double* xyz, const double* uv, int min_points,
                                const ccal_solver_opts* opts, double* poses_io, int32_t* status_out, int32_t* iters_out,
                                int32_t* n_used_out, double* cost0_out, double* cost_out, double* err_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    if (n_cams < 1 || n_cams > CCAL_MAX_CAMS) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_rig_poses_batch: n_cams outside 1 .. CCAL_MAX_CAMS");
    if (!model || !params || !extr) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_rig_poses_batch: NULL argument");
    for (int pass = 0; pass < 2; ++pass)          // an unknown id of any camera is reported ahead of EUCMT
        for (int c = 0; c < n_cams; ++c) {
            const int rc = pass || model[c] != CCAL_MODEL_EUCMT ? check_model(ctx, model[c], "ccal_refine_rig_poses_batch") : CCAL_OK;
            if (rc != CCAL_OK) return rc;
        }
    if (n_slots < 0) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_rig_poses_batch: n_slots < 0");
    if (n_slots == 0) return CCAL_OK;
    if (!seg_offsets || !poses_io || !status_out) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_rig_poses_batch: NULL argument");
    if (check_offsets(ctx, "ccal_refine_rig_poses_batch", "seg_offsets", seg_offsets, n_slots, 0)) return CCAL_ERR_INVALID_ARG;
    const size_t n_seg = (size_t)seg_offsets[n_slots], ns = (size_t)n_slots;
    if (n_seg && (!seg_cam || !pt_offsets)) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_rig_poses_batch: NULL argument");
    // segment by segment, its point offsets ahead of its camera: the offsets up to the first camera out of range, then that camera
    size_t j_cam = 0;
    while (j_cam < n_seg && seg_cam[j_cam] >= 0 && seg_cam[j_cam] < n_cams) ++j_cam;
    if (n_seg && check_offsets(ctx, "ccal_refine_rig_poses_batch", "pt_offsets", pt_offsets, std::min(j_cam + 1, n_seg), 0)) return CCAL_ERR_INVALID_ARG;
    if (j_cam < n_seg) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_rig_poses_batch: seg_cam out of range");
    for (int i = 0; i < n_slots && n_seg; ++i)
        if (pt_offsets[seg_offsets[i + 1]] - pt_offsets[seg_offsets[i]] > (1 << 24))
            return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_rig_poses_batch: at most 2^24 points in a slot");
    const size_t n_tot = n_seg ? (size_t)pt_offsets[n_seg] : 0;
    if (n_tot && (!xyz || !uv)) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_rig_poses_batch: NULL argument");
    CCAL_API_TRY
    // one block: segment offsets | point offsets | segment cameras | points | image points | poses, cost0, cost | errors |
    // status, iterations, counts
    CallBlock blk(ctx);
    const auto s_sof = blk.add<int64_t>(ns + 1);
    const auto s_pof = blk.add<int64_t>(n_seg + 1);
    const auto s_cam = blk.add<int32_t>(n_seg + 1);
    const auto s_xyz = blk.add<double>((n_tot + 1) * 3);
    const auto s_uv = blk.add<double>((n_tot + 1) * 2);
    const RefineResults res(blk, ns, n_tot, err_out != nullptr);
    if (!blk.alloc()) return blk.finish("ccal_refine_rig_poses_batch");
    RigRefineArgs a = {};
    for (int c = 0; c < n_cams; ++c) {
        canonical_theta(ctx, model[c], params + (size_t)c * CCAL_PMAX, a.th[c], &a.rt);
        for (int i = 0; i < 6; ++i) a.extr[c][i] = extr[(size_t)c * 6 + i];
        a.model[c] = model[c];
    }
    a.seg_off = blk.at(s_sof); a.pt_off = blk.at(s_pof); a.seg_cam = blk.at(s_cam); a.io.xyz = blk.at(s_xyz); a.io.uv = blk.at(s_uv);
    a.io.rule = refine_rule(huber_delta, opts, n_slots, min_points);
    blk.poison(s_xyz, res.s_err);
    blk.upload(s_sof, seg_offsets, ns + 1);
    blk.upload(s_pof, pt_offsets, n_seg ? n_seg + 1 : 0);
    blk.upload(s_cam, seg_cam, n_seg);
    blk.upload(s_xyz, xyz, n_tot * 3);
    blk.upload(s_uv, uv, n_tot * 2);
    res.start(a.io, poses_io);
    if (blk.ok()) {
        hipLaunchKernelGGL(k_rig_pose_refine, dim3((n_slots + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK), dim3(256), 0, ctx->stream, a);
        blk.launched();
    }
    res.download(a.io, poses_io, status_out, iters_out, n_used_out, cost0_out, cost_out, err_out);
    return blk.finish("ccal_refine_rig_poses_batch");
    CCAL_API_CATCH(ctx)
}

}  // extern "C"

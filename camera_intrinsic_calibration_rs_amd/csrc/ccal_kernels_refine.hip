// Pose refinement under fixed intrinsics (ccal_refine_poses_batch): the maximum-likelihood board pose of every frame of a batch,
// min over (rvec, tvec) of  sum_i rho(| project(theta, R X_i + t) - uv_i |^2)  with the Huber loss of the joint solve, the camera
// model frozen.  n_prob independent 6-unknown problems in ONE launch, one wavefront per frame, four per workgroup (the shape of
// k_pose_pnp), the whole Levenberg-Marquardt solve of a frame inside the launch:
//   pass     lanes stride the frame's corners: residual and its 2 x 6 Jacobian w.r.t. rvec | tvec (frame_setup<false> +
//            corner_block<MODEL, false, false>, ccal_device.hpp - the pose columns of the joint solve's block), Huber corrector
//            (huber_sqrt_weight), lane-private lower triangle of J^T J (21), J^T r (6) and the cost in f64; one xor-shuffle
//            butterfly leaves the same totals on all 64 lanes (a fixed order: nothing depends on the batch)
//   solve    every lane: (J^T J + lambda clamp(diag)) d = -J^T r by a 6 x 6 Cholesky in registers (the arithmetic of chol_solve_reg,
//            ccal_head.hpp) - wave-uniform, no LDS, no barrier
//   decide   the pass at pose + d gives the trial value (and, for an accepted step, the next system: one pass per iteration); the
//            trust-region rule of optimizer_decide (ccal_fused.hpp), one state per frame
// Steps are judged on  sum rho(s),  the function whose gradient J^T rho' r is, so that the iteration can reach its own fixed point;
// the cost REPORTED is the library's  sum rho'(s) s.  The two are the same function while no corner is beyond delta.  With outliers
// they differ (2 delta sqrt(s) - delta^2 against delta sqrt(s) per outlier), their minima lie apart, and a rule that judged the
// corrected Gauss-Newton step on the reported cost would stop between the two, at no stationary point of either.
// Nothing goes back to the host in between.  A corner whose projection is undefined at a pose gets no rule of its own: its
// residual is NaN and so is the cost, as in the joint solve - CCAL_ERR_NONFINITE at the start, a rejected step at a trial pose.
#include <algorithm>
#include <cmath>
#include "ccal_call.hpp"
#include "ccal_refine.hpp"

namespace ccal {

struct RefineArgs {
    double th[CCAL_PMAX];               // the camera's parameters in the kernels' canonical order
    ModelRt rt;
    const int64_t* off;                 // [n_prob + 1]
    RefineIO io;
};

// The pass, solve and decide steps, the count of valid points, both result stores and the host's result slices (RefineIO,
// RefineResults) are in ccal_refine.hpp, shared with the rig's kernel (ccal_kernels_rig_refine.hip).
template <int MODEL>
__global__ __launch_bounds__(256) void k_pose_refine(const RefineArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int o = blockIdx.x * WAVES_PER_BLOCK + wave;
    if (o >= a.io.rule.n_prob) return;
    const int64_t start = a.off[o];
    const int n = (int)(a.off[o + 1] - start);
    const double* xyz = a.io.xyz + 3 * start;
    const double* uv = a.io.uv + 2 * start;
    double* err = a.io.err ? a.io.err + start : nullptr;
    double th[th_len<MODEL>()];
    load_theta<MODEL, false>(a.th, a.rt, th);

    double pose[6];
    bool start_ok = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) { pose[i] = a.io.poses[(int64_t)o * 6 + i]; start_ok = start_ok && refine_finite(pose[i]); }
    int cnt = 0;
    for (int c = lane; c < n; c += 64) cnt += refine_point_valid(xyz, uv, c) ? 1 : 0;
    refine_count(cnt);
    if (!start_ok || cnt < refine_min_points(a.io)) {
        if (err) for (int c = lane; c < n; c += 64) err[c] = __builtin_nan("");
        refine_store_none(a.io, o, lane);
        return;
    }

    // one pass over the frame's corners at the pose p: the totals on all lanes
    const double delta = a.io.rule.delta;
    auto pass = [&](const double* p, const bool with_err, double* H, double* g, double& rep, double& obj) {
        double fc[FC_N0];
        frame_setup<false>(p, nullptr, fc);
        refine_zero(H, g, rep, obj);
        refine_corners<MODEL, false>(th, fc, xyz, uv, with_err ? err : nullptr, n, lane, delta, H, g, rep, obj);
        refine_reduce(H, g, rep, obj);
    };
    int iter;
    double cost0, cost;
    const int status = refine_lm(a.io.rule, err != nullptr, pass, pose, iter, cost0, cost);
    refine_store(a.io, o, lane, pose, status, iter, cnt, cost0, cost);
}

template <int M> struct LaunchRefine { static void go(int g, hipStream_t st, const RefineArgs& a) { hipLaunchKernelGGL(k_pose_refine<M>, dim3(g), dim3(256), 0, st, a); } };

}  // namespace ccal

using namespace ccal;

extern "C" {

int ccal_refine_poses_batch(ccal_ctx* ctx, int model, const double* params, double huber_delta, int n_prob, const int64_t* offsets,
                            const double* xyz, const double* uv, int min_points, const ccal_solver_opts* opts, double* poses_io,
                            int32_t* status_out, int32_t* iters_out, int32_t* n_used_out, double* cost0_out, double* cost_out,
                            double* err_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    const int rc = check_model(ctx, model, "ccal_refine_poses_batch");
    if (rc != CCAL_OK) return rc;
    if (n_prob < 0) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_poses_batch: n_prob < 0");
    if (!params) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_poses_batch: NULL argument");
    if (n_prob == 0) return CCAL_OK;
    if (!offsets || !poses_io || !status_out) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_poses_batch: NULL argument");
    if (check_offsets(ctx, "ccal_refine_poses_batch", "offsets", offsets, n_prob, 1 << 24)) return CCAL_ERR_INVALID_ARG;
    const size_t n_tot = (size_t)offsets[n_prob], np = (size_t)n_prob;
    if (n_tot && (!xyz || !uv)) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_poses_batch: NULL argument");
    CCAL_API_TRY
    // one block: offsets | points | image points | poses, cost0, cost | errors | status, iterations, counts
    CallBlock blk(ctx);
    const auto s_off = blk.add<int64_t>(np + 1);
    const auto s_xyz = blk.add<double>((n_tot + 1) * 3);
    const auto s_uv = blk.add<double>((n_tot + 1) * 2);
    const RefineResults res(blk, np, n_tot, err_out != nullptr);
    if (!blk.alloc()) return blk.finish("ccal_refine_poses_batch");
    RefineArgs a = {};
    canonical_theta(ctx, model, params, a.th, &a.rt);
    a.off = blk.at(s_off); a.io.xyz = blk.at(s_xyz); a.io.uv = blk.at(s_uv);
    a.io.rule = refine_rule(huber_delta, opts, n_prob, min_points);
    blk.poison(s_xyz, res.s_err);
    blk.upload(s_off, offsets, np + 1);
    blk.upload(s_xyz, xyz, n_tot * 3);
    blk.upload(s_uv, uv, n_tot * 2);
    res.start(a.io, poses_io);
    if (blk.ok()) {
        launch_model<LaunchRefine>(model, (n_prob + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, ctx->stream, a);
        blk.launched();
    }
    res.download(a.io, poses_io, status_out, iters_out, n_used_out, cost0_out, cost_out, err_out);
    return blk.finish("ccal_refine_poses_batch");
    CCAL_API_CATCH(ctx)
}

}  // extern "C"

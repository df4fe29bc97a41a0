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
#include <string>

#include "ccal_device.hpp"
#include "ccal_fused.hpp"
#include "ccal_internal.hpp"

namespace ccal {

struct RefineArgs {
    double th[CCAL_PMAX];               // the camera's parameters in the kernels' canonical order
    ModelRt rt;
    const int64_t* off;                 // [n_prob + 1]
    const double* xyz; const double* uv;     // [.][3], [.][2] pixels
    double* poses;                      // [n_prob][6] in: start, out: result
    int32_t* status; int32_t* iters; int32_t* n_used;
    double* cost0; double* cost;        // [n_prob]
    double* err;                        // [n_points] pixel error at the result, or nullptr
    double delta;
    double radius0, min_diag, max_diag, min_error, min_abs, min_rel;
    int32_t n_prob, min_points, max_iter, error_metric;
};

constexpr int kRefTri = 21;             // packed lower triangle of the 6 x 6 system: entry (i, j <= i) at i (i + 1) / 2 + j

__device__ __forceinline__ bool refine_finite(double v) { return fabs(v) < __builtin_inf(); }

// One pass over the frame's corners at `pose`: H = J^T J (packed lower), g = J^T r, cost = sum rho'(s) s, obj = sum rho(s), the same
// on all lanes.
// err != nullptr: also the pixel error of every corner (NaN for a corner that is left out).
template <int MODEL>
__device__ __forceinline__ void refine_pass(const double* th, const double* pose, const double* xyz, const double* uv, double* err,
                                            const int n, const int lane, const double delta, double* H, double* g, double& cost, double& obj) {
    constexpr int P = model_np(MODEL);
    double fc[FC_N0];
    frame_setup<false>(pose, nullptr, fc);
#pragma unroll
    for (int i = 0; i < kRefTri; ++i) H[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) g[i] = 0.0;
    cost = 0.0; obj = 0.0;
    for (int c = lane; c < n; c += 64) {
        const double X = xyz[3 * (int64_t)c], Y = xyz[3 * (int64_t)c + 1], Z = xyz[3 * (int64_t)c + 2];
        const double uo = uv[2 * (int64_t)c], vo = uv[2 * (int64_t)c + 1];
        const bool valid = refine_finite(X) && refine_finite(Y) && refine_finite(Z) && refine_finite(uo) && refine_finite(vo);
        if (!valid) {
            if (err) err[c] = __builtin_nan("");
            continue;
        }
        double ru, rv, Ju[P + 6], Jv[P + 6];
        corner_block<MODEL, false, false>(th, fc, X, Y, Z, uo, vo, ru, rv, Ju, Jv);
        const double s = ru * ru + rv * rv;
        if (err) err[c] = sqrt(s);
        const double sw = huber_sqrt_weight(s, delta);
        ru *= sw; rv *= sw;
        const double cs = ru * ru + rv * rv;            // rho'(s) s: s, or delta sqrt(s) for a corner beyond delta
        cost += cs;
        obj += (delta > 0.0 && s > delta * delta) ? 2.0 * cs - delta * delta : cs;      // rho(s): s, or 2 delta sqrt(s) - delta^2
        double a[6], b[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) { a[i] = sw * Ju[P + i]; b[i] = sw * Jv[P + i]; }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = 0; j <= i; ++j) H[i * (i + 1) / 2 + j] += a[i] * a[j] + b[i] * b[j];
            g[i] += a[i] * ru + b[i] * rv;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int i = 0; i < kRefTri; ++i) H[i] += __shfl_xor(H[i], off, 64);
#pragma unroll
        for (int i = 0; i < 6; ++i) g[i] += __shfl_xor(g[i], off, 64);
        cost += __shfl_xor(cost, off, 64);
        obj += __shfl_xor(obj, off, 64);
    }
}

// (H + diag(D)) d = -g by Cholesky, in registers (the arithmetic of chol_solve_reg).  false: not positive definite (d = 0).
__device__ __forceinline__ bool refine_solve(const double* H, const double* D, const double* g, double* d) {
    double M[kRefTri], v[6];
#pragma unroll
    for (int i = 0; i < kRefTri; ++i) M[i] = H[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) { M[i * (i + 1) / 2 + i] += D[i]; v[i] = -g[i]; }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double dj = M[j * (j + 1) / 2 + j];
#pragma unroll
        for (int k = 0; k < j; ++k) dj -= M[j * (j + 1) / 2 + k] * M[j * (j + 1) / 2 + k];
        ok = ok && (dj > 0.0) && (dj < 1.7e308);
        double sq, rs;
        fast_sqrt_rsqrt(ok ? dj : 1.0, sq, rs);
        M[j * (j + 1) / 2 + j] = rs;                       // inverted diagonal
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double t = M[i * (i + 1) / 2 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) t -= M[i * (i + 1) / 2 + k] * M[j * (j + 1) / 2 + k];
            M[i * (i + 1) / 2 + j] = t * rs;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double t = v[i];
#pragma unroll
        for (int k = 0; k < i; ++k) t -= M[i * (i + 1) / 2 + k] * v[k];
        v[i] = t * M[i * (i + 1) / 2 + i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double t = v[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) t -= M[k * (k + 1) / 2 + i] * v[k];
        v[i] = t * M[i * (i + 1) / 2 + i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) d[i] = ok ? v[i] : 0.0;
    return ok;
}

template <int MODEL>
__global__ __launch_bounds__(256) void k_pose_refine(const RefineArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int o = blockIdx.x * WAVES_PER_BLOCK + wave;
    if (o >= a.n_prob) return;
    const int64_t start = a.off[o];
    const int n = (int)(a.off[o + 1] - start);
    const double* xyz = a.xyz + 3 * start;
    const double* uv = a.uv + 2 * start;
    double* err = a.err ? a.err + start : nullptr;
    double th[th_len<MODEL>()];
    load_theta<MODEL, false>(a.th, a.rt, th);

    double pose[6], trial[6];
    bool start_ok = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) { pose[i] = a.poses[(int64_t)o * 6 + i]; trial[i] = pose[i]; start_ok = start_ok && refine_finite(pose[i]); }
    int cnt = 0;
    for (int c = lane; c < n; c += 64) {
        bool v = refine_finite(uv[2 * (int64_t)c]) && refine_finite(uv[2 * (int64_t)c + 1]);
#pragma unroll
        for (int k = 0; k < 3; ++k) v = v && refine_finite(xyz[3 * (int64_t)c + k]);
        cnt += v ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (!start_ok || cnt < (a.min_points > 3 ? a.min_points : 3)) {      // no result: the pose stays as the caller gave it
        if (err) for (int c = lane; c < n; c += 64) err[c] = __builtin_nan("");
        if (lane == 0) {
            a.status[o] = CCAL_NO_RESULT; a.iters[o] = 0; a.n_used[o] = 0; a.cost0[o] = 0.0; a.cost[o] = 0.0;
        }
        return;
    }

    // the frame's optimizer state (optimizer_decide's LM branch, ccal_fused.hpp, with the frame's own radius and stop rules)
    // cur: sum rho(s) at the accepted pose, what the steps and the stop rules are judged on; rep: the reported cost there
    double H[kRefTri], g[6], cur = 0.0, rep = 0.0, cost0 = 0.0;
    double radius = a.radius0, dec = 2.0, mc = 0.0;
    int iter = 0, done = 0;               // done: ccal_status + 1
    bool first = true, lin_ok = true, final_pass = false;
    const int em = a.error_metric;
    for (;;) {
        double Ht[kRefTri], gt[6], rt, ct;
        refine_pass<MODEL>(th, trial, xyz, uv, final_pass ? err : nullptr, n, lane, a.delta, Ht, gt, rt, ct);
        if (final_pass) break;
        bool accept = false;
        if (first) {
            first = false; accept = true; cost0 = rt;
            if (!(fabs(ct) < 1.7e308)) done = CCAL_ERR_NONFINITE + 1;
        } else {
            iter += 1;
            const double rho = (cur - ct) / mc;
            const bool fin = fabs(ct) < 1.7e308;
            const double mce = model_decrease_of(cur, mc, em);
            if (lin_ok && fin && mc >= 0.0 && (mce < a.min_abs || mce < a.min_rel * error_of(cur, em))) {
                // predicted decrease below the thresholds: converged
                accept = ct < cur;
                done = CCAL_OK + 1;
            } else if (lin_ok && fin && mc > 0.0 && rho > 0.0) {
                accept = true;
                const double t = 2.0 * rho - 1.0;
                radius = fmin(1e16, radius / fmax(1.0 / 3.0, 1.0 - t * t * t));
                dec = 2.0;
                const double le = error_of(cur, em), ce = error_of(ct, em);
                if (ce < a.min_error) done = CCAL_OK + 1;
                else if (fabs(le - ce) < a.min_abs) done = CCAL_OK + 1;
                else if (fabs(le - ce) / le < a.min_rel) done = CCAL_OK + 1;
            } else {
                radius /= dec; dec *= 2.0;
                if (radius < 1e-32) done = CCAL_ERR_NO_CONVERGENCE + 1;
            }
            if (!done && iter >= a.max_iter) done = CCAL_ERR_NO_CONVERGENCE + 1;
        }
        if (accept) {
            cur = ct; rep = rt;
#pragma unroll
            for (int i = 0; i < 6; ++i) { pose[i] = trial[i]; g[i] = gt[i]; }
#pragma unroll
            for (int i = 0; i < kRefTri; ++i) H[i] = Ht[i];
        }
        if (done) {
            if (!err) break;
            final_pass = true;
#pragma unroll
            for (int i = 0; i < 6; ++i) trial[i] = pose[i];
            continue;
        }
        // the damped step from the accepted point and its model decrease  d^T (D d - g)
        const double lambda = 1.0 / radius;
        double D[6], d[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) D[i] = lambda * fmin(fmax(H[i * (i + 1) / 2 + i], a.min_diag), a.max_diag);
        lin_ok = refine_solve(H, D, g, d);
        mc = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) { mc += d[i] * (D[i] * d[i] - g[i]); trial[i] = pose[i] + d[i]; }
    }
    if (lane == 0) {
        const bool nonfinite = done == CCAL_ERR_NONFINITE + 1;          // (the start itself: the pose stays, the costs are what they are)
#pragma unroll
        for (int i = 0; i < 6; ++i) a.poses[(int64_t)o * 6 + i] = pose[i];
        a.status[o] = done - 1; a.iters[o] = iter; a.n_used[o] = cnt;
        a.cost0[o] = cost0; a.cost[o] = nonfinite ? cost0 : rep;
    }
}

template <int MODEL>
static hipError_t launch_refine(const RefineArgs& a, hipStream_t s) {
    const int blocks = (a.n_prob + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pose_refine<MODEL>, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace ccal

using namespace ccal;

namespace {

int fail(ccal_ctx* ctx, int code, const char* msg) { note_error(ctx, msg); return code; }
int hip_fail(ccal_ctx* ctx, const char* where, hipError_t e) {
    try { ctx->err = std::string(where) + ": " + hipGetErrorString(e); } catch (...) { }
    return CCAL_ERR_HIP;
}
size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

int ccal_refine_poses_batch(ccal_ctx* ctx, int model, const double* params, double huber_delta, int n_prob, const int64_t* offsets,
                            const double* xyz, const double* uv, int min_points, const ccal_solver_opts* opts, double* poses_io,
                            int32_t* status_out, int32_t* iters_out, int32_t* n_used_out, double* cost0_out, double* cost_out,
                            double* err_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    if (model == CCAL_MODEL_EUCMT)
        return fail(ctx, CCAL_ERR_UNSUPPORTED, "ccal_refine_poses_batch: EUCMT is a parameter container in this build (its projection is only in the absent camera-intrinsic-model crate)");
    if (model < 0 || model >= kNumModels) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_poses_batch: unknown camera model");
    if (n_prob < 0) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_poses_batch: n_prob < 0");
    if (!params) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_poses_batch: NULL argument");
    if (n_prob == 0) return CCAL_OK;
    if (!offsets || !poses_io || !status_out) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_poses_batch: NULL argument");
    if (offsets[0] != 0) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_poses_batch: offsets[0] != 0");
    for (int i = 0; i < n_prob; ++i) {
        const int64_t n = offsets[i + 1] - offsets[i];
        if (n < 0 || n > (1 << 24)) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_poses_batch: offsets must not decrease, at most 2^24 points in a problem");
    }
    const size_t n_tot = (size_t)offsets[n_prob], np = (size_t)n_prob;
    if (n_tot && (!xyz || !uv)) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_refine_poses_batch: NULL argument");
    ccal_solver_opts o;
    if (opts) o = *opts; else ccal_set_defaults(&o);
    CCAL_API_TRY
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, "hipSetDevice", e);
    // one block: offsets | points | image points | poses, cost0, cost | errors | status, iterations, counts
    const size_t b_off = up256((np + 1) * 8), b_xyz = up256((n_tot + 1) * 24), b_uv = up256((n_tot + 1) * 16), b_res = up256(np * 8 * 8);
    const size_t b_err = err_out ? up256((n_tot + 1) * 8) : 0, b_int = up256(np * 3 * 4);
    char* d = nullptr;
    e = ctx_dev_alloc(ctx, (void**)&d, b_off + b_xyz + b_uv + b_res + b_err + b_int);
    if (e != hipSuccess) return hip_fail(ctx, "ccal_refine_poses_batch: allocation", e);
    struct Guard { ccal_ctx* c; char* p; ~Guard() { (void)hipStreamSynchronize(c->stream); ctx_release(c, p, false); } } guard{ ctx, d };
    RefineArgs a = {};
    for (int i = 0; i < model_np(model); ++i) a.th[i] = params[(model == kOCV5 && i >= 4) ? 4 + ctx->conv.ocv5_order[i - 4] : i];
    a.rt = model_rt(ctx);
    a.rt.ocv5_perm = kOcv5IdentityPerm;
    int64_t* d_off = (int64_t*)d;
    double* d_xyz = (double*)(d + b_off);
    double* d_uv = (double*)(d + b_off + b_xyz);
    double* d_po = (double*)(d + b_off + b_xyz + b_uv);
    double* d_err = err_out ? (double*)(d + b_off + b_xyz + b_uv + b_res) : nullptr;
    int32_t* d_int = (int32_t*)(d + b_off + b_xyz + b_uv + b_res + b_err);
    a.off = d_off; a.xyz = d_xyz; a.uv = d_uv;
    a.poses = d_po; a.cost0 = d_po + np * 6; a.cost = d_po + np * 7; a.err = d_err;
    a.status = d_int; a.iters = d_int + np; a.n_used = d_int + 2 * np;
    a.delta = huber_delta;
    a.radius0 = o.lm_initial_radius; a.min_diag = o.lm_min_diagonal; a.max_diag = o.lm_max_diagonal;
    a.min_error = o.min_error; a.min_abs = o.min_abs_error_decrease; a.min_rel = o.min_rel_error_decrease;
    a.n_prob = n_prob; a.min_points = min_points; a.max_iter = o.max_iterations; a.error_metric = o.error_metric ? 1 : 0;
    hipStream_t s = ctx->stream;
    e = test_poison_f64(ctx, d_xyz, b_xyz + b_uv + b_res + b_err, false, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_off, offsets, (np + 1) * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && n_tot) e = hipMemcpyAsync(d_xyz, xyz, n_tot * 24, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && n_tot) e = hipMemcpyAsync(d_uv, uv, n_tot * 16, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_po, poses_io, np * 6 * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        switch (model) {
            case kUCM: e = launch_refine<kUCM>(a, s); break;
            case kEUCM: e = launch_refine<kEUCM>(a, s); break;
            case kKB4: e = launch_refine<kKB4>(a, s); break;
            default: e = launch_refine<kOCV5>(a, s); break;
        }
    }
    if (e == hipSuccess) e = hipMemcpyAsync(poses_io, d_po, np * 6 * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(status_out, a.status, np * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && iters_out) e = hipMemcpyAsync(iters_out, a.iters, np * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && n_used_out) e = hipMemcpyAsync(n_used_out, a.n_used, np * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && cost0_out) e = hipMemcpyAsync(cost0_out, a.cost0, np * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && cost_out) e = hipMemcpyAsync(cost_out, a.cost, np * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && err_out && n_tot) e = hipMemcpyAsync(err_out, d_err, n_tot * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(ctx, "ccal_refine_poses_batch", e);
    return CCAL_OK;
    CCAL_API_CATCH(ctx)
}

}  // extern "C"

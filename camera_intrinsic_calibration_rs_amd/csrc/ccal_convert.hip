// util::convert_model (src/util.rs:224-282) with ModelConvertFactor (src/optimization/factors.rs:10-76):
// fit the target model's intrinsics so that it reproduces the source model over a pixel grid.
//   grid      rows/cols from edge = max(w,h)/100 in steps of max(w,h)/30            (util.rs:245-246, factors.rs:35-39)
//   rays      source.unproject(grid), the points it can unproject                   (factors.rs:40-44)
//   residual  ONE block of dimension 2 M: source.project(ray) - target.project(ray); 10000 where either
//             projection is undefined (factors.rs:58-73); HuberLoss(1.0) on the whole block (util.rs:252)
//   solve     Gauss-Newton on "params" = all target intrinsics, first four initialised from the source
//             (util.rs:256-258), the reference's bounds, last k distortion parameters fixed at 0 (util.rs:265-274)
// About 900 points and at most 9 unknowns: two small kernels (rays once; Gram per iteration on one workgroup,
// lane-private triangle + shuffle/LDS reduction, fixed order) and the 9 x 9 solve on the host.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <cstdio>
#include <string>

#include "ccal_call.hpp"
#include "ccal_device.hpp"
#include "ccal_host_gn.hpp"
#include "ccal_internal.hpp"
#include "ccal_model_inverse.hpp"

namespace ccal {

constexpr int CONV_REC = 6;          // x, y, z, u0, v0, state (0 dropped, 1 both projections defined so far, 2 source undefined)

struct ConvArgs {
    const double* src; const double* tgt;       // device copies of the parameter vectors
    double* rays;                               // [n_grid][CONV_REC]
    int32_t n_rows, n_cols, edge, steps;
    double* out;                                // [P (P+1)/2 | P | s | n_points]
    ModelRt rt;                                 // the context's conventions; the OPENCV5 order is the canonical one here: the
                                                // parameter vectors are permuted at the API boundary (ccal_convert_model)
};

template <int SRC>
__global__ __launch_bounds__(256) void k_convert_rays(const ConvArgs a) {
    const int n = a.n_rows * a.n_cols;
    double th[th_len<SRC>()];
    load_theta<SRC, false>(a.src, a.rt, th);
    for (int k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256) {
        const int r = a.edge + (k / a.n_cols) * a.steps, c = a.edge + (k % a.n_cols) * a.steps;
        double x = 0.0, y = 0.0, z = 0.0, u0 = 0.0, v0 = 0.0, state = 0.0;
        if (unproject_ray<SRC>(th, a.rt.unproject_eps, (double)c, (double)r, x, y, z)) {
            if (project_valid<SRC>(th, x, y, z)) { project_uv<SRC>(th, x, y, z, u0, v0); state = 1.0; }
            else state = 2.0;
        }
        double* o = a.rays + (int64_t)k * CONV_REC;
        o[0] = x; o[1] = y; o[2] = z; o[3] = u0; o[4] = v0; o[5] = state;
    }
}

template <int TGT>
__global__ __launch_bounds__(256) void k_convert_gram(const ConvArgs a) {
    constexpr int P = model_np(TGT), ND = P - 4, NT = P * (P + 1) / 2, NA = NT + P + 2;
    __shared__ double part[4][NA];
    double th[th_len<TGT>()];
    load_theta<TGT, false>(a.tgt, a.rt, th);
    double acc[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) acc[i] = 0.0;
    const int n = a.n_rows * a.n_cols;
    for (int k = threadIdx.x; k < n; k += 256) {
        const double* q = a.rays + (int64_t)k * CONV_REC;
        const double state = q[5];
        if (state == 0.0) continue;
        acc[NT + P + 1] += 1.0;
        const double x = q[0], y = q[1], z = q[2];
        if (state == 2.0 || !project_valid<TGT>(th, x, y, z)) { acc[NT + P] += 2.0 * 10000.0 * 10000.0; continue; }
        double mx, my, dmx[3], dmy[3], ddx[ND], ddy[ND];
        project_partials<TGT>(th, x, y, z, mx, my, dmx, dmy, ddx, ddy);
        // r = source - target, so dr/dtheta = -d(target)/dtheta
        double Ju[P], Jv[P];
        Ju[0] = -mx; Ju[1] = 0.0; Ju[2] = -1.0; Ju[3] = 0.0;
        Jv[0] = 0.0; Jv[1] = -my; Jv[2] = 0.0; Jv[3] = -1.0;
#pragma unroll
        for (int i = 0; i < ND; ++i) { Ju[4 + i] = -th[0] * ddx[i]; Jv[4 + i] = -th[1] * ddy[i]; }
        const double ru = q[3] - (th[0] * mx + th[2]), rv = q[4] - (th[1] * my + th[3]);
        int e = 0;
#pragma unroll
        for (int i = 0; i < P; ++i) {
#pragma unroll
            for (int j = 0; j <= i; ++j) { acc[e] += Ju[i] * Ju[j] + Jv[i] * Jv[j]; ++e; }
        }
#pragma unroll
        for (int i = 0; i < P; ++i) acc[NT + i] += Ju[i] * ru + Jv[i] * rv;
        acc[NT + P] += ru * ru + rv * rv;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        double v = acc[i];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) part[wave][i] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NA; i += 256) a.out[i] = (part[0][i] + part[1][i]) + (part[2][i] + part[3][i]);
}

namespace {
// bounds of set_problem_parameter_bound (src/util.rs:29-48); distortion part from the context's conventions table
void reference_bounds(const ccal_model_conventions& cv, int model, double w, double h, double* lo, double* hi) {
    lo[0] = 0.0; hi[0] = 10000.0; lo[1] = 0.0; hi[1] = 10000.0; lo[2] = 0.0; hi[2] = w; lo[3] = 0.0; hi[3] = h;
    for (int i = 4; i < model_np(model); ++i) { lo[i] = cv.dist_lo[model][i - 4]; hi[i] = cv.dist_hi[model][i - 4]; }
}
template <int M> struct LaunchRays { static void go(int g, hipStream_t st, const ConvArgs& a) { hipLaunchKernelGGL(k_convert_rays<M>, dim3(g), dim3(256), 0, st, a); } };
template <int M> struct LaunchGram { static void go(int g, hipStream_t st, const ConvArgs& a) { hipLaunchKernelGGL(k_convert_gram<M>, dim3(g), dim3(256), 0, st, a); } };
}  // namespace

}  // namespace ccal

using namespace ccal;

extern "C" int ccal_convert_model(ccal_ctx* ctx, int src_model, const double* src_params, int tgt_model,
                                  double* tgt_params_io, double width, double height, int disabled_distortions,
                                  const ccal_solver_opts* opts, ccal_report* rep) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    const int PS = ccal_model_num_params(src_model), P = ccal_model_num_params(tgt_model);
    if (PS < 0 || P < 0 || !src_params || !tgt_params_io || disabled_distortions < 0 || disabled_distortions > P - 4 ||
        !(width >= 1.0) || !(height >= 1.0)) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_convert_model: invalid argument");
    ccal_report R = {};
    if (src_model == kUCM && tgt_model == kEUCM) {                  // src/util.rs:229-235: closed form
        for (int i = 0; i < 5; ++i) tgt_params_io[i] = src_params[i];
        tgt_params_io[5] = 1.0;
        if (rep) *rep = R;
        return CCAL_OK;
    }
    if (src_model == kUCM && tgt_model == CCAL_MODEL_EUCMT) {      // src/util.rs:236-243: beta = 1, both tangential terms 0
        for (int i = 0; i < 5; ++i) tgt_params_io[i] = src_params[i];
        tgt_params_io[5] = 1.0; tgt_params_io[6] = 0.0; tgt_params_io[7] = 0.0;
        if (rep) *rep = R;
        return CCAL_OK;
    }
    // EUCMT is a parameter container here: its projection lives only in the absent camera-intrinsic-model crate
    if (src_model >= kNumModels || tgt_model >= kNumModels)
        return fail(ctx, CCAL_ERR_UNSUPPORTED, "ccal_convert_model: EUCMT can only be the target of the closed-form UCM conversion");
    ccal_solver_opts o;
    if (opts) o = *opts; else ccal_set_defaults(&o);
    const double big = std::max(width, height);
    const uint32_t edge = (uint32_t)big / 100u;
    const int steps = (int)(big / 30.0);
    if (steps < 1 || (uint32_t)height <= 2 * edge || (uint32_t)width <= 2 * edge) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_convert_model: image too small for the grid");
    const int n_rows = (int)(((uint32_t)height - 2 * edge + steps - 1) / steps);
    const int n_cols = (int)(((uint32_t)width - 2 * edge + steps - 1) / steps);
    const int n_grid = n_rows * n_cols;
    const int NT = P * (P + 1) / 2, NA = NT + P + 2;

    CallBlock blk(ctx);
    const auto s_src = blk.add<double>(CCAL_PMAX);
    const auto s_tgt = blk.add<double>(CCAL_PMAX);
    const auto s_out = blk.add<double>(64);
    const auto s_rays = blk.add<double>((size_t)n_grid * CONV_REC);
    if (!blk.alloc()) return blk.finish("ccal_convert_model");
    blk.poison(s_src, s_rays);
    // The fit runs in the kernels' canonical OPENCV5 order (k1, k2, p1, p2, k3): both parameter vectors are permuted HERE, at the
    // boundary (ccal_model_conventions.ocv5_order), the kernels get the identity
    ModelRt rt = model_rt(ctx);
    rt.ocv5_perm = kOcv5IdentityPerm;
    const int32_t* ord = ctx->conv.ocv5_order;
    auto canon = [&](int model, int i) { return (model == kOCV5 && i >= 4) ? 4 + ord[i - 4] : i; };     // canonical index -> caller's index
    const ConvArgs a{ blk.at(s_src), blk.at(s_tgt), blk.at(s_rays), n_rows, n_cols, (int32_t)edge, steps, blk.at(s_out), rt };

    double th[CCAL_PMAX] = { 0 }, lo[CCAL_PMAX], hi[CCAL_PMAX], src_c[CCAL_PMAX] = { 0 };
    for (int i = 0; i < PS; ++i) src_c[i] = src_params[canon(src_model, i)];
    for (int i = 0; i < P; ++i) th[i] = tgt_params_io[canon(tgt_model, i)];
    for (int i = 0; i < 4; ++i) th[i] = src_params[i];                      // util.rs:256-258
    bool fx[CCAL_PMAX] = { false };
    for (int i = 0; i < disabled_distortions; ++i) {                        // the LAST k of the caller's vector (src/util.rs:58-70)
        for (int c = 0; c < P; ++c) if (canon(tgt_model, c) == P - 1 - i) { fx[c] = true; th[c] = 0.0; }
    }
    reference_bounds(ctx->conv, tgt_model, width, height, lo, hi);

    blk.upload(s_src, src_c, (size_t)PS);
    if (blk.ok()) { launch_model<LaunchRays>(src_model, (n_grid + 255) / 256, ctx->stream, a); blk.launched(); }

    double out[64];
    auto eval = [&](const double* t) -> int {                              // the sums at t, waited for: CCAL_OK or the block's failure
        blk.upload(s_tgt, t, (size_t)P);
        if (blk.ok()) { launch_model<LaunchGram>(tgt_model, 1, ctx->stream, a); blk.launched(); }
        blk.download(out, a.out, (size_t)NA);
        return blk.finish("ccal_convert_model");
    };
    if (eval(th) != CCAL_OK) return CCAL_ERR_HIP;
    if (out[NT + P + 1] < 1.0) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_convert_model: the source model cannot unproject any grid point");
    double s = out[NT + P];
    double cur = huber_weight(s, 1.0) * s;
    R.initial_cost = cur;
    int status = CCAL_OK;
    if (!std::isfinite(cur)) status = CCAL_ERR_NONFINITE;
    for (int it = 0; status == CCAL_OK && it < o.max_iterations; ++it) {
        const double last = cur;
        const double w = huber_weight(s, 1.0);            // one block: the corrector is a common factor of H and g
        double S[81], dx[9];
        int e = 0;
        for (int i = 0; i < P; ++i) for (int j = 0; j <= i; ++j) { S[i * P + j] = S[j * P + i] = w * out[e]; ++e; }
        for (int i = 0; i < P; ++i) dx[i] = fx[i] ? 0.0 : -w * out[NT + i];
        for (int i = 0; i < P; ++i) if (fx[i]) { for (int j = 0; j < P; ++j) { S[i * P + j] = 0.0; S[j * P + i] = 0.0; } S[i * P + i] = 1.0; }
        if (!chol_factor(S, P)) { status = CCAL_ERR_NOT_PD; break; }
        chol_solve(S, P, dx);
        for (int i = 0; i < P; ++i) if (!fx[i]) th[i] = std::min(std::max(th[i] + dx[i], lo[i]), hi[i]);
        if (eval(th) != CCAL_OK) return CCAL_ERR_HIP;
        s = out[NT + P];
        cur = huber_weight(s, 1.0) * s;
        R.iterations++;
        if (o.verbose) std::printf("[ccal convert_model] iter %d cost %.12g\n", it, cur);
        const GnNext next = gn_decide(last, cur, o.error_metric, o.min_error, o.min_abs_error_decrease, o.min_rel_error_decrease);
        if (next == GnNext::nonfinite) status = CCAL_ERR_NONFINITE;
        if (next != GnNext::go_on) break;
        if (it == o.max_iterations - 1) status = CCAL_ERR_NO_CONVERGENCE;
    }
    R.final_cost = cur; R.status = status;
    if (rep) *rep = R;
    if (status == CCAL_OK || status == CCAL_ERR_NO_CONVERGENCE) for (int i = 0; i < P; ++i) tgt_params_io[canon(tgt_model, i)] = th[i];
    if (status != CCAL_OK && ctx->err.empty()) ctx->err = "ccal_convert_model: solve failed";
    return status;
    CCAL_API_CATCH(ctx)
}

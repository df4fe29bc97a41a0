// C ABI of the from-detections initialisation (include/ccal.h): the batched RANSAC of radial_distortion_homography
// (src/optimization/homography.rs:218-271; kernels in ccal_kernels_rdh.hip), homography_to_focal (:274-325, host code) and
// the division-model pose initialisation init_pose (src/optimization/linear.rs:5-21; k_pose_init's division variant), and the
// batched general PnP (sqpnp_solve_glam for many problems in one launch; k_pose_pnp, ccal_kernels_pnp.hip).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ccal_internal.hpp"
#include "ccal_rdh.hpp"

using namespace ccal;

namespace {

int fail(ccal_ctx* ctx, int code, const char* msg) { note_error(ctx, msg); return code; }
int hip_fail(ccal_ctx* ctx, const char* where, hipError_t e) {
    try { ctx->err = std::string(where) + ": " + hipGetErrorString(e); } catch (...) { }
    return CCAL_ERR_HIP;
}
size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// one of the two focal estimates of homography_to_focal: the larger of (va, vb) first; both positive: the one whose
// denominator of the ORIGINAL order is larger in magnitude selects first / second (homography.rs:291-301, 309-319)
bool focal_from(double va, double vb, double da, double db, double* f) {
    double v1 = va, v2 = vb;
    if (v1 < v2) { v1 = vb; v2 = va; }
    if (v1 > 0.0 && v2 > 0.0) { *f = std::sqrt(std::fabs(da) > std::fabs(db) ? v1 : v2); return true; }
    if (v1 > 0.0) { *f = std::sqrt(v1); return true; }
    return false;
}

}  // namespace

extern "C" {

int ccal_homography_to_focal(const double* H, double* f) {
    if (!H || !f) return CCAL_ERR_INVALID_ARG;
    const double h0 = H[0], h1 = H[1], h2 = H[2], h3 = H[3], h4 = H[4], h5 = H[5], h6 = H[6], h7 = H[7];
    double fa = 0.0, fb = 0.0;
    // from the third row: the two columns of H K are orthogonal and of equal norm
    const double d1 = h6 * h7, d2 = (h7 - h6) * (h7 + h6);
    const bool has_b = focal_from(-(h0 * h1 + h3 * h4) / d1, (h0 * h0 + h3 * h3 - h1 * h1 - h4 * h4) / d2, d1, d2, &fb);
    // from the first two rows
    const double e1 = h0 * h3 + h1 * h4, e2 = h0 * h0 + h1 * h1 - h3 * h3 - h4 * h4;
    const bool has_a = focal_from(-h2 * h5 / e1, (h5 * h5 - h2 * h2) / e2, e1, e2, &fa);
    if (has_a && has_b) *f = std::sqrt(fa * fb);
    else if (has_a) *f = fa;
    else if (has_b) *f = fb;
    else { *f = 0.0; return CCAL_NO_RESULT; }
    return CCAL_OK;
}

int ccal_rdh_batch(ccal_ctx* ctx, int n_prob, const int64_t* pair_offsets, const double* pairs, const uint64_t* seeds, int n_hyp,
                   double* lambda_out, double* H_out, double* score_out, int32_t* best_idx_out, int32_t* n_valid_out,
                   int32_t* hyp_sample, double* hyp_lambda, double* hyp_H, double* hyp_score) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    if (n_prob < 0 || n_prob > 65535 || n_hyp < 1 || n_hyp > (1 << 24)) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_rdh_batch: n_prob in 0..65535, n_hyp in 1..2^24");
    if (n_prob == 0) return CCAL_OK;
    if (!pair_offsets || !pairs || !seeds || !lambda_out || !H_out || !score_out || !best_idx_out || !n_valid_out) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_rdh_batch: NULL argument");
    int64_t max_pairs = 0;
    for (int i = 0; i < n_prob; ++i) {
        const int64_t n = pair_offsets[i + 1] - pair_offsets[i];
        if (n < 6) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_rdh_batch: a problem has fewer than 6 point pairs");
        if (n > (1 << 24)) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_rdh_batch: more than 2^24 pairs in a problem");
        max_pairs = std::max(max_pairs, n);
    }
    if (pair_offsets[0] != 0) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_rdh_batch: pair_offsets[0] != 0");
    const size_t n_tot = (size_t)pair_offsets[n_prob], np = (size_t)n_prob, nh = np * (size_t)n_hyp;
    const int n_blocks = (n_hyp + 63) / 64;
    if (nh > ((size_t)1 << 28)) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_rdh_batch: n_prob * n_hyp too large");
    CCAL_API_TRY
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, "hipSetDevice", e);
    // one block: inputs | workgroup records | results | per-hypothesis results (doubles first, then the 32-bit arrays)
    const size_t b_off = up256((np + 1) * 8), b_seed = up256(np * 8), b_pairs = up256(n_tot * 32), b_part = up256(np * (size_t)n_blocks * sizeof(RdhPartial));
    const size_t b_out = up256(np * 11 * 8), b_hl = hyp_lambda ? up256(nh * 8) : 0, b_hH = hyp_H ? up256(nh * 72) : 0, b_hs = hyp_score ? up256(nh * 8) : 0;
    const size_t b_oi = up256(np * 8), b_hsamp = hyp_sample ? up256(nh * 24) : 0;
    char* d = nullptr;
    e = ctx_dev_alloc(ctx, (void**)&d, b_off + b_seed + b_pairs + b_part + b_out + b_hl + b_hH + b_hs + b_oi + b_hsamp);
    if (e != hipSuccess) return hip_fail(ctx, "ccal_rdh_batch: allocation", e);
    struct Guard { ccal_ctx* c; char* p; ~Guard() { (void)hipStreamSynchronize(c->stream); ctx_release(c, p, false); } } guard{ ctx, d };
    char* q = d;
    int64_t* d_off = (int64_t*)q; q += b_off;
    uint64_t* d_seed = (uint64_t*)q; q += b_seed;
    double* d_pairs = (double*)q; q += b_pairs;
    RdhArgs a = {};
    a.part = (RdhPartial*)q; q += b_part;
    char* d_res = q;
    a.out_lambda = (double*)q; a.out_score = a.out_lambda + np; a.out_H = a.out_score + np; q += b_out;
    a.h_lambda = hyp_lambda ? (double*)q : nullptr; q += b_hl;
    a.h_H = hyp_H ? (double*)q : nullptr; q += b_hH;
    a.h_score = hyp_score ? (double*)q : nullptr; q += b_hs;
    a.out_idx = (int32_t*)q; a.out_nvalid = a.out_idx + np; q += b_oi;
    a.h_sample = hyp_sample ? (int32_t*)q : nullptr; q += b_hsamp;
    a.pair_off = d_off; a.seeds = d_seed; a.pairs = d_pairs; a.n_hyp = n_hyp; a.n_blocks = n_blocks;
    hipStream_t s = ctx->stream;
    e = test_poison_f64(ctx, d_res, b_out + b_hl + b_hH + b_hs, false, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_off, pair_offsets, (np + 1) * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_seed, seeds, np * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_pairs, pairs, n_tot * 32, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = launch_rdh(a, n_prob, (int)max_pairs, s);
    if (e == hipSuccess) e = hipMemcpyAsync(lambda_out, a.out_lambda, np * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(score_out, a.out_score, np * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(H_out, a.out_H, np * 72, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(best_idx_out, a.out_idx, np * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(n_valid_out, a.out_nvalid, np * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && hyp_lambda) e = hipMemcpyAsync(hyp_lambda, a.h_lambda, nh * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && hyp_H) e = hipMemcpyAsync(hyp_H, a.h_H, nh * 72, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && hyp_score) e = hipMemcpyAsync(hyp_score, a.h_score, nh * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && hyp_sample) e = hipMemcpyAsync(hyp_sample, a.h_sample, nh * 24, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(ctx, "ccal_rdh_batch", e);
    return CCAL_OK;
    CCAL_API_CATCH(ctx)
}

int ccal_radial_distortion_homography(ccal_ctx* ctx, const double* pairs, int n_pairs, uint64_t seed, int n_hyp,
                                      double* lambda_out, double* H_out, double* score_out, int32_t* best_idx_out, int32_t* n_valid_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    if (!best_idx_out || !n_valid_out) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_radial_distortion_homography: NULL argument");
    const int64_t off[2] = { 0, n_pairs };
    const int rc = ccal_rdh_batch(ctx, 1, off, pairs, &seed, n_hyp, lambda_out, H_out, score_out, best_idx_out, n_valid_out,
                                  nullptr, nullptr, nullptr, nullptr);
    if (rc != CCAL_OK) return rc;
    return *n_valid_out > 0 ? CCAL_OK : fail(ctx, CCAL_NO_RESULT, "ccal_radial_distortion_homography: no hypothesis had an admissible root");
}

int ccal_init_poses_division(ccal_problem* p, double lambda, int min_points, double* poses_obs, int32_t* n_used) {
    if (!p || !poses_obs || !n_used) return CCAL_ERR_INVALID_ARG;
    ccal_ctx* ctx = p->ctx;
    if (!(lambda == lambda)) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_init_poses_division: lambda is NaN");
    CCAL_API_TRY
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, "hipSetDevice", e);
    const size_t no = (size_t)std::max(p->n_obs, 1);
    const size_t b_po = up256(no * 6 * sizeof(double)), b_va = up256(no * sizeof(int32_t));
    char* d = nullptr;
    e = ctx_dev_alloc(ctx, (void**)&d, b_po + b_va);
    if (e != hipSuccess) return hip_fail(ctx, "ccal_init_poses_division: allocation", e);
    struct Guard { ccal_ctx* c; char* p; ~Guard() { (void)hipStreamSynchronize(c->stream); ctx_release(c, p, false); } } guard{ ctx, d };
    double* d_po = (double*)d; int32_t* d_va = (int32_t*)(d + b_po);
    e = test_poison_f64(ctx, d_po, b_po, false, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_va, 0, no * sizeof(int32_t), ctx->stream);
    for (int c = 0; c < p->n_cams && e == hipSuccess; ++c) e = launch_pose_init_division(p, c, lambda, d_po, d_va, min_points, ctx->stream);
    if (e == hipSuccess && p->n_obs) {
        e = hipMemcpyAsync(poses_obs, d_po, (size_t)p->n_obs * 6 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(n_used, d_va, (size_t)p->n_obs * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, "ccal_init_poses_division", e);
    return CCAL_OK;
    CCAL_API_CATCH(ctx)
}

int ccal_pnp_batch(ccal_ctx* ctx, int n_prob, const int64_t* offsets, const double* xyz, const double* xn, int min_points,
                   double* poses_out, int32_t* n_used_out, double* cost_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    if (n_prob < 0) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_pnp_batch: n_prob < 0");
    if (n_prob == 0) return CCAL_OK;
    if (!offsets || !poses_out || !n_used_out) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_pnp_batch: NULL argument");
    if (offsets[0] != 0) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_pnp_batch: offsets[0] != 0");
    for (int i = 0; i < n_prob; ++i) {
        const int64_t n = offsets[i + 1] - offsets[i];
        if (n < 0 || n > (1 << 24)) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_pnp_batch: offsets must not decrease, at most 2^24 points in a problem");
    }
    const size_t n_tot = (size_t)offsets[n_prob], np = (size_t)n_prob;
    if (n_tot && (!xyz || !xn)) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_pnp_batch: NULL argument");
    CCAL_API_TRY
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, "hipSetDevice", e);
    // one block: offsets | points | image points | poses, costs | counts
    const size_t b_off = up256((np + 1) * 8), b_xyz = up256((n_tot + 1) * 24), b_xn = up256((n_tot + 1) * 16), b_res = up256(np * 7 * 8), b_nu = up256(np * 4);
    char* d = nullptr;
    e = ctx_dev_alloc(ctx, (void**)&d, b_off + b_xyz + b_xn + b_res + b_nu);
    if (e != hipSuccess) return hip_fail(ctx, "ccal_pnp_batch: allocation", e);
    struct Guard { ccal_ctx* c; char* p; ~Guard() { (void)hipStreamSynchronize(c->stream); ctx_release(c, p, false); } } guard{ ctx, d };
    int64_t* d_off = (int64_t*)d;
    double* d_xyz = (double*)(d + b_off);
    double* d_xn = (double*)(d + b_off + b_xyz);
    double* d_po = (double*)(d + b_off + b_xyz + b_xn);
    double* d_cost = d_po + np * 6;
    int32_t* d_nu = (int32_t*)(d + b_off + b_xyz + b_xn + b_res);
    hipStream_t s = ctx->stream;
    e = test_poison_f64(ctx, d_po, b_res, false, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_off, offsets, (np + 1) * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && n_tot) e = hipMemcpyAsync(d_xyz, xyz, n_tot * 24, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && n_tot) e = hipMemcpyAsync(d_xn, xn, n_tot * 16, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = launch_pnp_batch(n_prob, d_off, d_xyz, d_xn, min_points, d_po, d_nu, d_cost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(poses_out, d_po, np * 6 * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(n_used_out, d_nu, np * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && cost_out) e = hipMemcpyAsync(cost_out, d_cost, np * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(ctx, "ccal_pnp_batch", e);
    return CCAL_OK;
    CCAL_API_CATCH(ctx)
}

}  // extern "C"

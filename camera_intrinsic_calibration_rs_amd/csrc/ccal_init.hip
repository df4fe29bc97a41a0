// C ABI of the from-detections initialisation (include/ccal.h): the batched RANSAC of radial_distortion_homography
// (src/optimization/homography.rs:218-271; kernels in ccal_kernels_rdh.hip), homography_to_focal (:274-325, host code) and
// the division-model pose initialisation init_pose (src/optimization/linear.rs:5-21; k_pose_init's division variant), and the
// batched general PnP (sqpnp_solve_glam for many problems in one launch; k_pose_pnp, ccal_kernels_pnp.hip).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ccal_call.hpp"
#include "ccal_rdh.hpp"

using namespace ccal;

namespace {

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
    if (check_offsets(ctx, "ccal_rdh_batch", "pair_offsets", pair_offsets, 0, 0)) return CCAL_ERR_INVALID_ARG;      // (the spans: above)
    const size_t n_tot = (size_t)pair_offsets[n_prob], np = (size_t)n_prob, nh = np * (size_t)n_hyp;
    const int n_blocks = (n_hyp + 63) / 64;
    if (nh > ((size_t)1 << 28)) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_rdh_batch: n_prob * n_hyp too large");
    CCAL_API_TRY
    // one block: inputs | workgroup records | results | per-hypothesis results (doubles first, then the 32-bit arrays)
    CallBlock blk(ctx);
    const auto s_off = blk.add<int64_t>(np + 1);
    const auto s_seed = blk.add<uint64_t>(np);
    const auto s_pairs = blk.add<double>(n_tot * 4);
    const auto s_part = blk.add<RdhPartial>(np * (size_t)n_blocks);
    const auto s_out = blk.add<double>(np * 11);                         // lambda | score | H
    const auto s_hl = blk.add<double>(hyp_lambda ? nh : 0);
    const auto s_hH = blk.add<double>(hyp_H ? nh * 9 : 0);
    const auto s_hs = blk.add<double>(hyp_score ? nh : 0);
    const auto s_oi = blk.add<int32_t>(np * 2);                          // best index | valid hypotheses
    const auto s_hsamp = blk.add<int32_t>(hyp_sample ? nh * 6 : 0);
    if (!blk.alloc()) return blk.finish("ccal_rdh_batch");
    RdhArgs a = {};
    a.pair_off = blk.at(s_off); a.seeds = blk.at(s_seed); a.pairs = blk.at(s_pairs); a.part = blk.at(s_part);
    a.out_lambda = blk.at(s_out); a.out_score = a.out_lambda + np; a.out_H = a.out_score + np;
    a.h_lambda = blk.at(s_hl); a.h_H = blk.at(s_hH); a.h_score = blk.at(s_hs);
    a.out_idx = blk.at(s_oi); a.out_nvalid = a.out_idx + np;
    a.h_sample = blk.at(s_hsamp);
    a.n_hyp = n_hyp; a.n_blocks = n_blocks;
    blk.poison(s_out, s_hs);
    blk.upload(s_off, pair_offsets, np + 1);
    blk.upload(s_seed, seeds, np);
    blk.upload(s_pairs, pairs, n_tot * 4);
    if (blk.ok()) blk.note(launch_rdh(a, n_prob, (int)max_pairs, ctx->stream));
    blk.download(lambda_out, a.out_lambda, np);
    blk.download(score_out, a.out_score, np);
    blk.download(H_out, a.out_H, np * 9);
    blk.download(best_idx_out, a.out_idx, np);
    blk.download(n_valid_out, a.out_nvalid, np);
    blk.download(hyp_lambda, a.h_lambda, nh);
    blk.download(hyp_H, a.h_H, nh * 9);
    blk.download(hyp_score, a.h_score, nh);
    blk.download(hyp_sample, a.h_sample, nh * 6);
    return blk.finish("ccal_rdh_batch");
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
    const size_t no = (size_t)std::max(p->n_obs, 1), n_obs = (size_t)p->n_obs;
    CallBlock blk(ctx);
    const auto s_po = blk.add<double>(no * 6);
    const auto s_va = blk.add<int32_t>(no);
    if (!blk.alloc()) return blk.finish("ccal_init_poses_division");
    blk.poison(s_po, s_po);
    blk.memset(s_va, 0, no);
    for (int c = 0; c < p->n_cams && blk.ok(); ++c) blk.note(launch_pose_init_division(p, c, lambda, blk.at(s_po), blk.at(s_va), min_points, ctx->stream));
    blk.download(poses_obs, blk.at(s_po), n_obs * 6);
    blk.download(n_used, blk.at(s_va), n_obs);
    return blk.finish("ccal_init_poses_division");
    CCAL_API_CATCH(ctx)
}

int ccal_pnp_batch(ccal_ctx* ctx, int n_prob, const int64_t* offsets, const double* xyz, const double* xn, int min_points,
                   double* poses_out, int32_t* n_used_out, double* cost_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    if (n_prob < 0) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_pnp_batch: n_prob < 0");
    if (n_prob == 0) return CCAL_OK;
    if (!offsets || !poses_out || !n_used_out) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_pnp_batch: NULL argument");
    if (check_offsets(ctx, "ccal_pnp_batch", "offsets", offsets, n_prob, 1 << 24)) return CCAL_ERR_INVALID_ARG;
    const size_t n_tot = (size_t)offsets[n_prob], np = (size_t)n_prob;
    if (n_tot && (!xyz || !xn)) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_pnp_batch: NULL argument");
    CCAL_API_TRY
    // one block: offsets | points | image points | poses, costs | counts
    CallBlock blk(ctx);
    const auto s_off = blk.add<int64_t>(np + 1);
    const auto s_xyz = blk.add<double>((n_tot + 1) * 3);
    const auto s_xn = blk.add<double>((n_tot + 1) * 2);
    const auto s_res = blk.add<double>(np * 7);                          // poses | cost
    const auto s_nu = blk.add<int32_t>(np);
    if (!blk.alloc()) return blk.finish("ccal_pnp_batch");
    double* d_po = blk.at(s_res);
    double* d_cost = d_po + np * 6;
    blk.poison(s_res, s_res);
    blk.upload(s_off, offsets, np + 1);
    blk.upload(s_xyz, xyz, n_tot * 3);
    blk.upload(s_xn, xn, n_tot * 2);
    if (blk.ok()) blk.note(launch_pnp_batch(n_prob, blk.at(s_off), blk.at(s_xyz), blk.at(s_xn), min_points, d_po, blk.at(s_nu), d_cost, ctx->stream));
    blk.download(poses_out, d_po, np * 6);
    blk.download(n_used_out, blk.at(s_nu), np);
    blk.download(cost_out, d_cost, np);
    return blk.finish("ccal_pnp_batch");
    CCAL_API_CATCH(ctx)
}

}  // extern "C"

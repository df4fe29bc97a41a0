// ccal_covariance (include/ccal.h, "calibration uncertainty"): the covariance of the camera block, of every board pose, and the
// leverage of every corner, from the loss-corrected Jacobian mode E leaves in the problem's d_r / d_J.
//
//   mode E (loss applied)      the existing launch, into p->d_r / p->d_J
//   k_cov_blocks               two wavefronts per observation frame: V_o (21), W_o (camera columns x 6), sum r^2 -> a record
//   k_cov_sum                  the cost: 128 workgroups over contiguous ranges, then one over their sums; fixed order
//   k_cov_slots<false>         one wavefront per slot: V_s = sum of its frames' V_o, Cholesky with the pivot rule -> the slot's verdict
//   host                       S of ccal_build_normal_dev(p, 0), fixed columns out, Cholesky + inverse in f64, S^-1 back to the device
//   k_cov_slots<true>          per slot: V^-1, Y_o = W_o V^-1, G_o = sum_o' S^-1[cols(o), cols(o')] Y_o', C = V^-1 + sum_o Y_o^T G_o,
//                              sigma2 C; then, lanes over the corners of each of its frames, a Sd a^T - 2 a G_o b^T + b C b^T
//   k_cov_sum                  the leverage sum
// Every sum runs in a fixed order (a lane's own loop, then a fixed tree): no atomics, the same bits from run to run.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "ccal_call.hpp"
#include "ccal_host_gn.hpp"
#include "ccal_normal.hpp"

using namespace ccal;

namespace {

constexpr double kPivotRel = 0x1p-36;          // a pivot at or below this x its own diagonal entry: not positive definite
constexpr int kRec = kCovRec, kNC = kCovCamCols, kYG = 6 * kCovCamCols;

struct CovCams { int32_t D[CCAL_MAX_CAMS], Peff[CCAL_MAX_CAMS], col_theta[CCAL_MAX_CAMS], col_extr[CCAL_MAX_CAMS]; };

struct CovArgs {
    const double* J; const double* r;
    const int64_t* obs_off; const int64_t* joff; const int32_t* obs_cam;
    const int32_t* slot_off; const int32_t* slot_obs;
    CovCams cams;
    int32_t n_obs, n_slots, K;
    double sigma2;
    double* rec;                   // [n_obs][kRec]
    const double* sinv;            // [K][K]
    double* pose_cov;              // [n_slots][36]
    double* lev;                   // [n_corners]
    int32_t* status;               // [n_slots]: 0 posed, 1 no corner, 2 V_s not positive definite
};

// row-major lower triangle
__host__ __device__ constexpr int tri(int i, int j) { return i * (i + 1) / 2 + j; }
// entry e of the lower triangle -> (i, j)
__device__ inline void tri_ij(int e, int& i, int& j) {
    i = 0;
    while (tri(i + 1, 0) <= e) ++i;
    j = e - tri(i, 0);
}
// the block's column of camera column c (theta, then - behind the six pose columns - the extrinsic)
__device__ inline int block_col(int c, int Peff) { return c < Peff ? c : c + 6; }
// the reduced system's column of camera column c of camera `cam`
__device__ inline int system_col(const CovCams& cm, int cam, int c) { return c < cm.Peff[cam] ? cm.col_theta[cam] + c : cm.col_extr[cam] + (c - cm.Peff[cam]); }

// One workgroup of two wavefronts per observation frame.  The frame's rows go through LDS a tile of 32 at a time (the block is
// row-major: a tile is one contiguous, coalesced read); thread e owns entry e of the record and walks the tile's rows in order from
// LDS - threads of a wavefront read a few columns of the same row, mostly as broadcasts - with two interleaved partial sums (even and
// odd rows) added at the end.
constexpr int kTileRows = 32;
__global__ __launch_bounds__(128) void k_cov_blocks(CovArgs a) {
    __shared__ double sJ[kTileRows * (kNC + 6)];
    __shared__ double sR[kTileRows];
    const int o = blockIdx.x, e = threadIdx.x;
    if (o >= a.n_obs) return;
    const int cam = a.obs_cam[o], D = a.cams.D[cam], Pe = a.cams.Peff[cam], NC = D - 6;
    const int64_t c0 = a.obs_off[o];
    const int rows = 2 * (int)(a.obs_off[o + 1] - c0);          // (even: two rows per corner)
    const double* J = a.J + a.joff[o];
    const double* r = a.r + 2 * c0;
    int ci = 0, cj = 0;
    bool live = e < kRec;
    if (e < 21) { int i, j; tri_ij(e, i, j); ci = Pe + i; cj = Pe + j; }
    else if (e < kRec - 1) { const int c = (e - 21) / 6; live = c < NC; ci = block_col(c, Pe); cj = Pe + (e - 21) % 6; }
    double s0 = 0.0, s1 = 0.0;
    for (int k0 = 0; k0 < rows; k0 += kTileRows) {
        const int nr = min(kTileRows, rows - k0);               // (even)
        for (int i = e; i < nr * D; i += 128) sJ[i] = J[(int64_t)k0 * D + i];
        for (int i = e; i < nr; i += 128) sR[i] = r[k0 + i];
        __syncthreads();
        if (live) {
            if (e == kRec - 1) {
                for (int k = 0; k < nr; k += 2) { s0 = fma(sR[k], sR[k], s0); s1 = fma(sR[k + 1], sR[k + 1], s1); }
            } else {
                for (int k = 0; k < nr; k += 2) {
                    s0 = fma(sJ[k * D + ci], sJ[k * D + cj], s0);
                    s1 = fma(sJ[(k + 1) * D + ci], sJ[(k + 1) * D + cj], s1);
                }
            }
        }
        __syncthreads();
    }
    if (e < kRec) a.rec[(int64_t)o * kRec + e] = s0 + s1;
}

// out[blockIdx.x] = the sum of the workgroup's share of n values `stride` apart - a contiguous range of ceil(n / gridDim.x) values:
// thread t adds the range's values t, t + 1024, ... in order, then a fixed tree.  Two launches make a sum: kSumBlocks partial sums,
// then one workgroup over those.
constexpr int kSumBlocks = 128;
__global__ __launch_bounds__(1024) void k_cov_sum(const double* src, int64_t stride, int64_t n, double* out) {
    __shared__ double part[1024];
    const int t = threadIdx.x;
    const int64_t share = (n + gridDim.x - 1) / gridDim.x, lo = (int64_t)blockIdx.x * share, hi = lo + share < n ? lo + share : n;
    double s = 0.0;
    for (int64_t i = lo + t; i < hi; i += 1024) s += src[i * stride];
    part[t] = s;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if (t < w) part[t] += part[t + w];
        __syncthreads();
    }
    if (t == 0) out[blockIdx.x] = part[0];
}
// d_sums: [0] cost, [1] leverage sum, [8 ..) the partial sums
static void enqueue_sum(hipStream_t st, const double* src, int64_t stride, int64_t n, double* d_sums, int which) {
    hipLaunchKernelGGL(k_cov_sum, dim3(kSumBlocks), dim3(1024), 0, st, src, stride, n, d_sums + 8);
    hipLaunchKernelGGL(k_cov_sum, dim3(1), dim3(1024), 0, st, d_sums + 8, (int64_t)1, (int64_t)kSumBlocks, d_sums + which);
}

// One wavefront per slot (a workgroup of 64).  The small matrices live in LDS and are read as broadcasts; the 6 x 6 factorisation
// and inverse run in every lane alike, on registers, with compile-time indices.
template <bool FULL>
__global__ __launch_bounds__(64) void k_cov_slots(CovArgs a) {
    __shared__ double sV[36], sVi[36], sC[36], sY[CCAL_MAX_CAMS * kYG], sG[CCAL_MAX_CAMS * kYG], sSd[kNC * kNC];
    const int s = blockIdx.x, lane = threadIdx.x;
    if (s >= a.n_slots) return;
    const int o0 = a.slot_off[s], m = min(a.slot_off[s + 1] - o0, CCAL_MAX_CAMS);        // one frame per (camera, slot)
    int64_t corners = 0;
    for (int t = 0; t < m; ++t) { const int o = a.slot_obs[o0 + t]; corners += a.obs_off[o + 1] - a.obs_off[o]; }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (corners == 0) {
        if (FULL) { if (lane < 36) a.pose_cov[(int64_t)s * 36 + lane] = nan; }
        else if (lane == 0) a.status[s] = 1;
        return;
    }
    if (lane < 21) {
        double v = 0.0;
        for (int t = 0; t < m; ++t) v += a.rec[(int64_t)a.slot_obs[o0 + t] * kRec + lane];
        int i, j; tri_ij(lane, i, j);
        sV[i * 6 + j] = v; sV[j * 6 + i] = v;
    }
    __syncthreads();
    // V = L L^T
    double L[21];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const double d = sV[j * 6 + j];
        double p = d;
#pragma unroll
        for (int k = 0; k < j; ++k) p -= L[tri(j, k)] * L[tri(j, k)];
        if (!(p > kPivotRel * d)) ok = false;
        const double l = sqrt(p);
        L[tri(j, j)] = l;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double t = sV[i * 6 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) t -= L[tri(i, k)] * L[tri(j, k)];
            L[tri(i, j)] = t / l;
        }
    }
    if (!FULL) { if (lane == 0) a.status[s] = ok ? 0 : 2; return; }
    if (!ok) { if (lane < 36) a.pose_cov[(int64_t)s * 36 + lane] = nan; return; }      // (the host has stopped at the verdict already)
    // M = L^-1, V^-1 = M^T M
    double M[21];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        M[tri(i, i)] = 1.0 / L[tri(i, i)];
#pragma unroll
        for (int j = 0; j < i; ++j) {
            double t = 0.0;
#pragma unroll
            for (int k = j; k < i; ++k) t -= L[tri(i, k)] * M[tri(k, j)];
            M[tri(i, j)] = t / L[tri(i, i)];
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                double t = 0.0;
#pragma unroll
                for (int k = i; k < 6; ++k) t += M[tri(k, i)] * M[tri(k, j)];
                sVi[i * 6 + j] = t; sVi[j * 6 + i] = t;
            }
        }
    }
    __syncthreads();
    // Y_o = W_o V^-1
    for (int t = 0; t < m; ++t) {
        const int o = a.slot_obs[o0 + t], NC = a.cams.D[a.obs_cam[o]] - 6;
        const double* W = a.rec + (int64_t)o * kRec + 21;
        for (int e = lane; e < kYG; e += 64) {
            const int c = e / 6, q = e % 6;
            double y = 0.0;
            if (c < NC) for (int k = 0; k < 6; ++k) y = fma(W[c * 6 + k], sVi[k * 6 + q], y);
            sY[t * kYG + e] = y;
        }
    }
    __syncthreads();
    // G_o = sum_o' S^-1[cols(o), cols(o')] Y_o'
    for (int t = 0; t < m; ++t) {
        const int cam = a.obs_cam[a.slot_obs[o0 + t]], NC = a.cams.D[cam] - 6;
        for (int e = lane; e < kYG; e += 64) {
            const int c = e / 6, q = e % 6;
            double g = 0.0;
            if (c < NC) {
                const double* row = a.sinv + (int64_t)system_col(a.cams, cam, c) * a.K;
                for (int t2 = 0; t2 < m; ++t2) {
                    const int cam2 = a.obs_cam[a.slot_obs[o0 + t2]], NC2 = a.cams.D[cam2] - 6;
                    for (int c2 = 0; c2 < NC2; ++c2) g = fma(row[system_col(a.cams, cam2, c2)], sY[t2 * kYG + c2 * 6 + q], g);
                }
            }
            sG[t * kYG + e] = g;
        }
    }
    __syncthreads();
    // C = V^-1 + sum_o Y_o^T G_o
    if (lane < 21) {
        int i, j; tri_ij(lane, i, j);
        double c = sVi[i * 6 + j];
        for (int t = 0; t < m; ++t) {
            const int NC = a.cams.D[a.obs_cam[a.slot_obs[o0 + t]]] - 6;
            for (int k = 0; k < NC; ++k) c = fma(sY[t * kYG + k * 6 + i], sG[t * kYG + k * 6 + j], c);
        }
        sC[i * 6 + j] = c; sC[j * 6 + i] = c;
        a.pose_cov[(int64_t)s * 36 + i * 6 + j] = a.sigma2 * c; a.pose_cov[(int64_t)s * 36 + j * 6 + i] = a.sigma2 * c;
    }
    __syncthreads();
    // the leverage of every corner of the slot's frames
    for (int t = 0; t < m; ++t) {
        const int o = a.slot_obs[o0 + t], cam = a.obs_cam[o], D = a.cams.D[cam], Pe = a.cams.Peff[cam], NC = D - 6;
        for (int e = lane; e < kNC * kNC; e += 64) {
            const int i = e / kNC, j = e % kNC;
            sSd[e] = (i < NC && j < NC) ? a.sinv[(int64_t)system_col(a.cams, cam, i) * a.K + system_col(a.cams, cam, j)] : 0.0;
        }
        __syncthreads();
        const int64_t c0 = a.obs_off[o];
        const int n = (int)(a.obs_off[o + 1] - c0);
        const double* J = a.J + a.joff[o];
        const double* G = sG + t * kYG;
        for (int k = lane; k < n; k += 64) {
            double h = 0.0;
#pragma unroll
            for (int row = 0; row < 2; ++row) {
                const double* Jr = J + (int64_t)(2 * k + row) * D;
                double av[kNC], bv[6];
#pragma unroll
                for (int i = 0; i < kNC; ++i) av[i] = i < NC ? Jr[block_col(i, Pe)] : 0.0;
#pragma unroll
                for (int q = 0; q < 6; ++q) bv[q] = Jr[Pe + q];
                // row i of a matrix at a time, from LDS (a broadcast), against the vector in registers; the row's own factor a_i / b_i
                // comes from the Jacobian again (a register array must not be indexed by a loop variable: it would go to scratch)
                double q = 0.0;
#pragma unroll 1
                for (int i = 0; i < NC; ++i) {
                    double u = 0.0, w = 0.0;
#pragma unroll
                    for (int j = 0; j < kNC; ++j) u = fma(sSd[i * kNC + j], av[j], u);
#pragma unroll
                    for (int p6 = 0; p6 < 6; ++p6) w = fma(G[i * 6 + p6], bv[p6], w);
                    q = fma(Jr[block_col(i, Pe)], u - 2.0 * w, q);
                }
#pragma unroll 1
                for (int i = 0; i < 6; ++i) {
                    double u = 0.0;
#pragma unroll
                    for (int j = 0; j < 6; ++j) u = fma(sC[i * 6 + j], bv[j], u);
                    q = fma(Jr[Pe + i], u, q);
                }
                h += q;
            }
            a.lev[c0 + k] = h;
        }
        __syncthreads();
    }
}

// S (K x K, the caller's order) without the fixed columns -> S^-1 with zero rows and columns in their place.  false: a pivot at or below
// kPivotRel x its own diagonal entry.  Cholesky (ccal_host_gn.hpp's loop with that pivot rule), M = L^-1, S^-1 = M^T M.
bool invert_free(const std::vector<double>& S, int K, const std::vector<int>& free_cols, std::vector<double>& Sinv) {
    const int n = (int)free_cols.size();
    std::vector<double> A((size_t)n * n), M((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) A[(size_t)i * n + j] = S[(size_t)free_cols[i] * K + free_cols[j]];
    for (int j = 0; j < n; ++j) {
        const double d = A[(size_t)j * n + j];
        double s = d;
        for (int k = 0; k < j; ++k) s -= A[(size_t)j * n + k] * A[(size_t)j * n + k];
        if (!(s > kPivotRel * d) || !std::isfinite(s)) return false;
        const double l = std::sqrt(s);
        A[(size_t)j * n + j] = l;
        for (int i = j + 1; i < n; ++i) {
            double t = A[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) t -= A[(size_t)i * n + k] * A[(size_t)j * n + k];
            A[(size_t)i * n + j] = t / l;
        }
    }
    for (int i = 0; i < n; ++i) {
        M[(size_t)i * n + i] = 1.0 / A[(size_t)i * n + i];
        for (int j = 0; j < i; ++j) {
            double t = 0.0;
            for (int k = j; k < i; ++k) t -= A[(size_t)i * n + k] * M[(size_t)k * n + j];
            M[(size_t)i * n + j] = t / A[(size_t)i * n + i];
        }
    }
    Sinv.assign((size_t)K * K, 0.0);
    for (int i = 0; i < n; ++i) for (int j = 0; j <= i; ++j) {
        double t = 0.0;
        for (int k = i; k < n; ++k) t += M[(size_t)k * n + i] * M[(size_t)k * n + j];
        Sinv[(size_t)free_cols[i] * K + free_cols[j]] = t; Sinv[(size_t)free_cols[j] * K + free_cols[i]] = t;
    }
    return true;
}

}  // namespace

extern "C" int ccal_covariance(ccal_problem* p, const double* intr, const double* poses, const double* extr, double* cov_cam,
                               double* cov_poses, double* leverage, int32_t* slot_status, ccal_cov_report* report) {
    if (!p) return CCAL_ERR_INVALID_ARG;
    ccal_ctx* ctx = p->ctx;
    if (!report) return fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_covariance: report is NULL");
    *report = ccal_cov_report{};
    report->bad_slot = -1;
    auto done = [&](int rc) { report->status = rc; return rc; };
    CCAL_API_TRY
    if (p->sharded()) return done(fail(ctx, CCAL_ERR_UNSUPPORTED, "ccal_covariance: a sharded problem holds a part of the frames only"));
    if (!cov_cam) return done(fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_covariance: cov_cam is NULL"));
    if (intr && !poses && p->n_slots) return done(fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_covariance: poses is NULL"));
    if (intr && !extr && p->n_cams > 1) return done(fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_covariance: extr is NULL"));
    const int K = p->K, n_slots = p->n_slots, n_obs = p->n_obs;
    // the slot -> observation frames table (frames of a slot need not be adjacent), the posed slots, the free columns
    std::vector<int32_t> slot_off((size_t)n_slots + 1, 0), slot_obs((size_t)std::max(n_obs, 1), 0);
    std::vector<int64_t> slot_corners((size_t)std::max(n_slots, 1), 0);
    for (int o = 0; o < n_obs; ++o) { slot_off[(size_t)p->h_obs_slot[o] + 1] += 1; slot_corners[p->h_obs_slot[o]] += p->h_obs_off[o + 1] - p->h_obs_off[o]; }
    for (int s = 0; s < n_slots; ++s) slot_off[(size_t)s + 1] += slot_off[s];
    {
        std::vector<int32_t> at(slot_off.begin(), slot_off.end() - 1);
        for (int o = 0; o < n_obs; ++o) slot_obs[at[p->h_obs_slot[o]]++] = o;
    }
    int n_posed = 0;
    for (int s = 0; s < n_slots; ++s) n_posed += slot_corners[s] > 0;
    std::vector<int> free_cols;
    for (int c = 0; c < p->n_cams; ++c) {
        const CamLayout& cl = p->cams[c];
        for (int i = 0; i < cl.Peff; ++i) if (!p->fixed[(size_t)c * CCAL_PMAX + i]) free_cols.push_back(cl.col_theta + i);
        if (c > 0) for (int i = 0; i < 6; ++i) free_cols.push_back(cl.col_extr + i);
    }
    report->n_posed = n_posed;
    report->n_free = (int32_t)free_cols.size() + 6 * n_posed;
    report->dof = 2 * p->n_corners - report->n_free;
    if (report->dof <= 0) return done(fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_covariance: no degrees of freedom left (2 x corners <= free parameters)"));

    HIP_TRY_RET(ctx, hipSetDevice(ctx->device), done(CCAL_ERR_HIP));
    int rc = CCAL_OK;
    if (intr && (rc = ccal_upload_params(p, intr, poses, extr)) != CCAL_OK) return done(rc);
    hipStream_t st = ctx->stream;
    const CovLayout l((size_t)p->n_corners, (size_t)n_obs, (size_t)n_slots, (size_t)K);
    const bool fresh = !p->d_cov;
    if (fresh) HIP_TRY_RET(ctx, ctx_block_alloc(ctx, l.plan, &p->d_cov, false), done(CCAL_ERR_HIP));
    const Bound dev{ p->d_cov };
    if (fresh) {          // the table: once (the vectors live until the synchronisation below)
        HIP_TRY_RET(ctx, hipMemcpyAsync(dev.at(l.slot_off), slot_off.data(), slot_off.size() * sizeof(int32_t), hipMemcpyHostToDevice, st), done(CCAL_ERR_HIP));
        HIP_TRY_RET(ctx, hipMemcpyAsync(dev.at(l.slot_obs), slot_obs.data(), slot_obs.size() * sizeof(int32_t), hipMemcpyHostToDevice, st), done(CCAL_ERR_HIP));
    }
    HIP_TRY_RET(ctx, ctx_doubles(ctx, &p->d_r, (size_t)std::max<int64_t>(2 * p->n_corners, 2)), done(CCAL_ERR_HIP));
    HIP_TRY_RET(ctx, ctx_doubles(ctx, &p->d_J, (size_t)std::max<int64_t>(p->j_len, 2)), done(CCAL_ERR_HIP));
    if ((rc = ccal_eval_dev(p, 1, p->d_r, p->d_J)) != CCAL_OK) return done(rc);

    CovArgs a = {};
    a.J = p->d_J; a.r = p->d_r; a.obs_off = p->d_obs_off; a.joff = p->d_joff; a.obs_cam = p->d_obs_cam;
    a.slot_off = dev.at(l.slot_off); a.slot_obs = dev.at(l.slot_obs);
    for (int c = 0; c < p->n_cams; ++c) {
        a.cams.D[c] = p->cams[c].D; a.cams.Peff[c] = p->cams[c].Peff; a.cams.col_theta[c] = p->cams[c].col_theta; a.cams.col_extr[c] = p->cams[c].col_extr;
    }
    a.n_obs = n_obs; a.n_slots = n_slots; a.K = K;
    a.rec = dev.at(l.rec); a.sinv = dev.at(l.sinv); a.pose_cov = dev.at(l.pose_cov); a.lev = dev.at(l.lev); a.status = dev.at(l.status);
    double* d_sums = dev.at(l.sums);
    std::vector<int32_t> status((size_t)std::max(n_slots, 1), 0);
    double sums[2] = { 0.0, 0.0 };
    if (n_obs > 0) hipLaunchKernelGGL(k_cov_blocks, dim3(n_obs), dim3(128), 0, st, a);
    enqueue_sum(st, a.rec + (kRec - 1), (int64_t)kRec, (int64_t)n_obs, d_sums, 0);
    if (n_slots > 0) hipLaunchKernelGGL(k_cov_slots<false>, dim3(n_slots), dim3(64), 0, st, a);
    HIP_TRY_RET(ctx, hipGetLastError(), done(CCAL_ERR_HIP));
    if (n_slots > 0) HIP_TRY_RET(ctx, hipMemcpyAsync(status.data(), a.status, (size_t)n_slots * sizeof(int32_t), hipMemcpyDeviceToHost, st), done(CCAL_ERR_HIP));
    HIP_TRY_RET(ctx, hipMemcpyAsync(&sums[0], d_sums, sizeof(double), hipMemcpyDeviceToHost, st), done(CCAL_ERR_HIP));
    HIP_TRY_RET(ctx, hipStreamSynchronize(st), done(CCAL_ERR_HIP));
    report->cost = sums[0];
    report->sigma2 = sums[0] / (double)report->dof;
    for (int s = 0; s < n_slots; ++s) if (status[s] == 2) {
        report->bad_slot = s;
        return done(fail(ctx, CCAL_ERR_NOT_PD, "ccal_covariance: a slot's pose block is not positive definite (report->bad_slot)"));
    }

    // S of mode N at lambda = 0, the fixed columns out, inverted on the host (K < 128)
    if ((rc = ccal_build_normal_dev(p, 0.0)) != CCAL_OK) return done(rc);
    std::vector<double> S((size_t)K * K), Sinv;
    if ((rc = normal_readback(p, 0.0, S.data(), nullptr, nullptr)) != CCAL_OK) return done(rc);
    if (!invert_free(S, K, free_cols, Sinv))
        return done(fail(ctx, CCAL_ERR_NOT_PD, "ccal_covariance: the reduced camera system is not positive definite"));
    HIP_TRY_RET(ctx, hipMemcpyAsync(dev.at(l.sinv), Sinv.data(), Sinv.size() * sizeof(double), hipMemcpyHostToDevice, st), done(CCAL_ERR_HIP));
    a.sigma2 = report->sigma2;
    if (n_slots > 0) hipLaunchKernelGGL(k_cov_slots<true>, dim3(n_slots), dim3(64), 0, st, a);
    enqueue_sum(st, a.lev, (int64_t)1, (int64_t)p->n_corners, d_sums, 1);
    HIP_TRY_RET(ctx, hipGetLastError(), done(CCAL_ERR_HIP));
    HIP_TRY_RET(ctx, hipMemcpyAsync(&sums[1], d_sums + 1, sizeof(double), hipMemcpyDeviceToHost, st), done(CCAL_ERR_HIP));
    if (cov_poses && n_slots > 0) HIP_TRY_RET(ctx, hipMemcpyAsync(cov_poses, a.pose_cov, (size_t)n_slots * 36 * sizeof(double), hipMemcpyDeviceToHost, st), done(CCAL_ERR_HIP));
    if (leverage && p->n_corners > 0) HIP_TRY_RET(ctx, hipMemcpyAsync(leverage, a.lev, (size_t)p->n_corners * sizeof(double), hipMemcpyDeviceToHost, st), done(CCAL_ERR_HIP));
    HIP_TRY_RET(ctx, hipStreamSynchronize(st), done(CCAL_ERR_HIP));
    report->leverage_sum = sums[1];
    for (size_t i = 0; i < Sinv.size(); ++i) cov_cam[i] = report->sigma2 * Sinv[i];
    if (slot_status) for (int s = 0; s < n_slots; ++s) slot_status[s] = status[s];
    return done(CCAL_OK);
    CCAL_API_CATCH(ctx)
}

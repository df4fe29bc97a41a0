// RANSAC for a homography with one-parameter division distortion between two views of the board: the loop of
// radial_distortion_homography (src/optimization/homography.rs:218-271) over its six-point minimal solver (:19-167) and its
// score (:169-216), for n_prob independent problems in one launch.
//
//   p ~ (x, y, 1 + l r^2),  p' ~ (x', y', 1 + l' r'^2),  p' ~ H p.
//   Eliminating the third row: x' (H1 . p) - y' (H0 . p) = 0 is linear in (h00 h01 h02 h10 h11 h12 l*h02 l*h12): a 6 x 8 system
//   with a two-dimensional null space n0, n1 (Householder QR of its transpose: the last two columns of Q).  v = g n0 + n1 is a
//   solution when v6 / v2 = v7 / v5 (= l): a quadratic in g.  Per root the third row of H and l' follow from the 6 x 4 least
//   squares system of the first row's equation; the admissible root has l, l' < 0 (the closer pair on a log scale when both
//   do), lambda = -sqrt(l l').  The result does not depend on which orthonormal basis of the null space is used.
//
// Mapping: one hypothesis per lane - the solve needs no cross-lane traffic; 64-thread workgroups (one wavefront), blockIdx.y = the
// problem, so that 1 000 hypotheses of one problem spread over 16 CUs.  The pairs of the problem are staged once in LDS and read as
// same-address broadcasts in the scoring loop (problems with more than RDH_LDS_PAIRS pairs read them from global memory at
// wave-uniform addresses instead).  Every array below is indexed by compile-time constants after unrolling: registers, no scratch.
// (score, index) is reduced per wavefront by shuffles into one record per workgroup; k_rdh_pick reduces the records of a problem.
// The winner is the lowest score, ties to the lowest hypothesis index: a pure function of (pairs, seed, n_hyp).
//
// Sampling: 6 distinct pair indices by a partial Fisher-Yates shuffle of 0 .. n_pairs-1 driven by the counter-based splitmix64 of
// synth.splitmix64(seed, 6, stream = hypothesis index) - api.rdh_sample_indices is its host twin.  (The reference shuffles with an
// unseeded generator.)  All arithmetic is f64 (the reference: f32).
#include "ccal_internal.hpp"
#include "ccal_rdh.hpp"

namespace ccal {

__device__ __forceinline__ uint64_t rdh_splitmix(uint64_t base, int k) {
    uint64_t z = base + (uint64_t)k * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// partial Fisher-Yates without the array: only the (at most six) positions a swap has written are remembered
__device__ __forceinline__ void rdh_sample(uint64_t seed, int hyp, int n, int* s) {
    const uint64_t base = seed + (uint64_t)hyp * 0xD1B54A32D192ED03ull;
    int mpos[6], mval[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int j = i + (int)(rdh_splitmix(base, i + 1) % (uint64_t)(n - i));
        int vi = i, vj = j;
#pragma unroll
        for (int q = 0; q < i; ++q) {
            if (mpos[q] == i) vi = mval[q];
            if (mpos[q] == j) vj = mval[q];
        }
        s[i] = vj;
        mpos[i] = j; mval[i] = vi;
    }
}

// Householder reflections of the first K columns of a (R x C, row-major in registers), applied to the columns behind them.
// The reflection vectors stay in place (rows k .. R-1 of column k), beta[k] = 2 / v.v (0: nothing to reflect), diag[k] = R[k][k].
template <int R, int C, int K>
__device__ __forceinline__ void householder(double (&a)[R][C], double (&beta)[K], double (&diag)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = 0.0;
#pragma unroll
        for (int i = k; i < R; ++i) s += a[i][k] * a[i][k];
        const double nrm = sqrt(s);
        const double alpha = a[k][k] > 0.0 ? -nrm : nrm;
        a[k][k] -= alpha;
        const double vv = s - alpha * (a[k][k] + alpha) ;             // v.v = 2 (s - alpha x_k)
        const double b = nrm > 0.0 ? 1.0 / vv : 0.0;                  // beta / 2 folded below
        beta[k] = b; diag[k] = alpha;
#pragma unroll
        for (int j = k + 1; j < C; ++j) {
            double d = 0.0;
#pragma unroll
            for (int i = k; i < R; ++i) d += a[i][k] * a[i][j];
            d *= b;
#pragma unroll
            for (int i = k; i < R; ++i) a[i][j] -= d * a[i][k];
        }
    }
}

struct RdhHyp { double lambda, H[9], score; bool valid; };

// the six-point solve: pairs q[6][4] = (x, y, x', y')
__device__ __forceinline__ bool rdh_solve(const double (&q)[6][4], double& lambda, double (&H)[9]) {
    double n0[8], n1[8];
    {
        double a[8][6], beta[6], diag[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const double x = q[r][0], y = q[r][1], xp = q[r][2], yp = q[r][3], r2 = x * x + y * y;
            a[0][r] = -x * yp; a[1][r] = -y * yp; a[2][r] = -yp;
            a[3][r] = x * xp;  a[4][r] = y * xp;  a[5][r] = xp;
            a[6][r] = -r2 * yp; a[7][r] = r2 * xp;
        }
        householder<8, 6, 6>(a, beta, diag);
        // n0 = Q e6, n1 = Q e7 with Q = H0 H1 .. H5
#pragma unroll
        for (int i = 0; i < 8; ++i) { n0[i] = i == 6 ? 1.0 : 0.0; n1[i] = i == 7 ? 1.0 : 0.0; }
#pragma unroll
        for (int k = 5; k >= 0; --k) {
            double d0 = 0.0, d1 = 0.0;
#pragma unroll
            for (int i = k; i < 8; ++i) { d0 += a[i][k] * n0[i]; d1 += a[i][k] * n1[i]; }
            d0 *= beta[k]; d1 *= beta[k];
#pragma unroll
            for (int i = k; i < 8; ++i) { n0[i] -= d0 * a[i][k]; n1[i] -= d1 * a[i][k]; }
        }
    }
    const double qa = n0[6] * n0[5] - n0[7] * n0[2];
    const double qb = n0[6] * n1[5] + n1[6] * n0[5] - n0[7] * n1[2] - n1[7] * n0[2];
    const double qc = n1[6] * n1[5] - n1[7] * n1[2];
    const double disc = qb * qb - 4.0 * qa * qc;
    if (!(disc >= 0.0)) return false;
    const double sq = sqrt(disc);
    double l[2], lp[2], Hc[2][9];
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        const double g = (w == 0 ? qb - sq : qb + sq) / (-2.0 * qa);          // root order of homography.rs:69-72
        double v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = g * n0[i] + n1[i];
        const double lw = v[6] / v[2];
        // first-row equation per pair: unknowns (h20, h21, h22, l'), 6 x 4 least squares by Householder on [A | b]
        double a[6][5], beta[4], diag[4];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const double x = q[r][0], y = q[r][1], xp = q[r][2], yp = q[r][3];
            const double sc = 1.0 + lw * (x * x + y * y);
            const double t = v[0] * x + v[1] * y + v[2] * sc;
            a[r][0] = -x * xp; a[r][1] = -y * xp; a[r][2] = -xp * sc; a[r][3] = (xp * xp + yp * yp) * t; a[r][4] = -t;
        }
        householder<6, 5, 4>(a, beta, diag);
        double sol[4];
#pragma unroll
        for (int i = 3; i >= 0; --i) {
            double t = a[i][4];
#pragma unroll
            for (int j = i + 1; j < 4; ++j) t -= a[i][j] * sol[j];
            sol[i] = t / diag[i];
        }
        l[w] = lw; lp[w] = sol[3];
#pragma unroll
        for (int i = 0; i < 6; ++i) Hc[w][i] = v[i];
        Hc[w][6] = sol[0]; Hc[w][7] = sol[1]; Hc[w][8] = sol[2];
    }
    const bool ok0 = l[0] < 0.0 && lp[0] < 0.0, ok1 = l[1] < 0.0 && lp[1] < 0.0;
    if (!ok0 && !ok1) return false;
    int pick;
    if (ok0 && ok1) pick = fabs(log10(l[0] / lp[0])) < fabs(log10(l[1] / lp[1])) ? 0 : 1;
    else pick = ok0 ? 0 : 1;
    lambda = -sqrt((pick ? l[1] : l[0]) * (pick ? lp[1] : lp[0]));
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = pick ? Hc[1][i] : Hc[0][i];
    return true;
}

// distance of one pair (homography.rs:179-207); which < 0: choose the branch of alpha on this pair
__device__ __forceinline__ double rdh_dist(const double (&H)[9], double lambda, double x, double y, double xp, double yp, int& which) {
    const double sc = 1.0 + lambda * (x * x + y * y);
    const double r0 = H[0] * x + H[1] * y + H[2] * sc;
    const double r1 = H[3] * x + H[4] * y + H[5] * sc;
    const double r2 = H[6] * x + H[7] * y + H[8] * sc;
    const double root = sqrt(fmax(-4.0 * lambda * (r0 * r0 + r1 * r1) + r2 * r2, 0.0));
    const double a0 = 0.5 * r2 - 0.5 * root, a1 = 0.5 * r2 + 0.5 * root;
    if (which < 0) which = fabs(xp - r0 / a0) < fabs(xp - r0 / a1) ? 0 : 1;
    const double al = which ? a1 : a0;
    const double dx = xp - r0 / al, dy = yp - r1 / al;
    return sqrt(dx * dx + dy * dy);
}

__device__ __forceinline__ bool rdh_better(double sa, int ia, double sb, int ib) { return sa < sb || (sa == sb && ia < ib); }

template <bool LDS>
__global__ __launch_bounds__(64) void k_rdh_hyp(const RdhArgs a) {
    extern __shared__ double s_pairs[];
    const int lane = threadIdx.x, prob = blockIdx.y;
    const int64_t start = a.pair_off[prob];
    const int n = (int)(a.pair_off[prob + 1] - start);
    const double* gp = a.pairs + 4 * start;
    if constexpr (LDS) {
        for (int i = lane; i < 4 * n; i += 64) s_pairs[i] = gp[i];
        __syncthreads();
    }
    const int hyp = blockIdx.x * 64 + lane;
    const int64_t slot = (int64_t)prob * a.n_hyp + hyp;
    double lambda = 0.0, H[9], score = INFINITY;
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = 0.0;
    bool valid = false;
    if (hyp < a.n_hyp && n >= 6) {
        int s[6];
        rdh_sample(a.seeds[prob], hyp, n, s);
        double q[6][4];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
            for (int c = 0; c < 4; ++c) q[r][c] = LDS ? s_pairs[4 * s[r] + c] : gp[4 * s[r] + c];
        }
        if (a.h_sample) {
#pragma unroll
            for (int r = 0; r < 6; ++r) a.h_sample[6 * slot + r] = s[r];
        }
        valid = rdh_solve(q, lambda, H);
        if (valid) {
            int which = -1;
            double sum = 0.0;
            for (int p = 0; p < n; ++p) {
                const double* pp = LDS ? &s_pairs[4 * p] : &gp[4 * p];
                sum += rdh_dist(H, lambda, pp[0], pp[1], pp[2], pp[3], which);
            }
            score = sum / (double)n;
            valid = score < INFINITY;                    // NaN or inf: no hypothesis (`avg_distance < best_distance` never holds)
        }
        if (!valid) {
            lambda = 0.0; score = INFINITY;
#pragma unroll
            for (int i = 0; i < 9; ++i) H[i] = 0.0;
        }
        if (a.h_lambda) a.h_lambda[slot] = lambda;
        if (a.h_score) a.h_score[slot] = score;
        if (a.h_H) {
#pragma unroll
            for (int i = 0; i < 9; ++i) a.h_H[9 * slot + i] = H[i];
        }
    }
    // the wavefront's winner: butterfly on (score, index); every lane ends with the same pair
    double bs = score; int bi = hyp, nv = valid ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double os = __shfl_xor(bs, off, 64); const int oi = __shfl_xor(bi, off, 64);
        if (rdh_better(os, oi, bs, bi)) { bs = os; bi = oi; }
        nv += __shfl_xor(nv, off, 64);
    }
    if (bi == hyp) {                                     // exactly one lane: indices are distinct
        RdhPartial* out = a.part + (int64_t)prob * gridDim.x + blockIdx.x;
        out->score = bs; out->lambda = lambda;
#pragma unroll
        for (int i = 0; i < 9; ++i) out->H[i] = H[i];
        out->idx = bi; out->n_valid = nv;
    }
}

// one wavefront per problem over its n_blocks records
__global__ __launch_bounds__(64) void k_rdh_pick(const RdhArgs a) {
    const int lane = threadIdx.x, prob = blockIdx.x;
    const RdhPartial* part = a.part + (int64_t)prob * a.n_blocks;
    double bs = INFINITY; int bi = INT_MAX, bb = 0, nv = 0;
    for (int b = lane; b < a.n_blocks; b += 64) {
        const double s = part[b].score; const int i = part[b].idx;
        if (rdh_better(s, i, bs, bi)) { bs = s; bi = i; bb = b; }
        nv += part[b].n_valid;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double os = __shfl_xor(bs, off, 64); const int oi = __shfl_xor(bi, off, 64), ob = __shfl_xor(bb, off, 64);
        if (rdh_better(os, oi, bs, bi)) { bs = os; bi = oi; bb = ob; }
        nv += __shfl_xor(nv, off, 64);
    }
    if (lane != 0) return;
    const bool any = nv > 0 && bs < INFINITY;
    a.out_lambda[prob] = any ? part[bb].lambda : 0.0;
    for (int i = 0; i < 9; ++i) a.out_H[9 * prob + i] = any ? part[bb].H[i] : 0.0;
    a.out_score[prob] = any ? bs : INFINITY;
    a.out_idx[prob] = any ? bi : -1;
    a.out_nvalid[prob] = nv;
}

hipError_t launch_rdh(const RdhArgs& a, int n_prob, int max_pairs, hipStream_t s) {
    if (n_prob <= 0 || a.n_hyp <= 0) return hipSuccess;
    const dim3 grid((unsigned)a.n_blocks, (unsigned)n_prob);
    if (max_pairs <= RDH_LDS_PAIRS) hipLaunchKernelGGL(k_rdh_hyp<true>, grid, dim3(64), (size_t)max_pairs * 4 * sizeof(double), s, a);
    else hipLaunchKernelGGL(k_rdh_hyp<false>, grid, dim3(64), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rdh_pick, dim3((unsigned)n_prob), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace ccal

// Second library only (libccal_hip_legacy.so, -DCCAL_LEGACY_KERNELS): the single-camera kernels that the register Gram kernels
// and their fused tail superseded for every model and size.  The parity tests keep them as the independent second
// implementation they hold the product kernels against:
//   k_gram1         the matrix-core Gram of round 1 (CCAL_GRAM=mfma)
//   k_schur1m       the separate elimination launch (behind k_gram1 and CCAL_FUSE_ELIM=0); tools/count_flops.py reads the
//                   elimination's operation count off its ISA
// Everything they share with the product kernels (corner_block, frame_setup, eliminate_frame, the record layout) is in the headers.
#include "ccal_device.hpp"
#include "ccal_fused.hpp"
#include "ccal_gram_common.hpp"

namespace ccal {

// ---------------------------------------------------------------------------------------------
// k_gram1
// ---------------------------------------------------------------------------------------------
template <int MODEL, bool OF>
__global__ __launch_bounds__(256, CCAL_GRAM_MINW) void k_gram1(const FusedArgs a) {
    constexpr int D = block_dim(MODEL, OF, false);
    constexpr int K = D - 6, K1 = K + 1;
    constexpr int RS = 16, CS = 2 * RS + 2;
    constexpr int WS = FC_N0P + GRAM_TILE_CORNERS * CS;
    extern __shared__ double smem[];
    const DevState* st = a.st;
    if (st->done || st->redo) return;            // finished, or a re-elimination group (no evaluation)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f = blockIdx.x * WAVES_PER_BLOCK + wave;
    if (f >= a.n_obs) return;
    double* fc = smem + wave * WS;
    double* tile = fc + FC_N0P;
    const int cur = st->cur, first = st->first;
    const int es = first ? cur : (cur ^ 1);
    const double* th_g = a.intr[es];
    double th[th_len<MODEL>()];
    load_theta<MODEL, OF>(th_g, a.rt, th);
    const int64_t start = a.obs_off[f];
    const int n = (int)(a.obs_off[f + 1] - start);
    // software prefetch: the first pass's corner rows are requested before the (long, latency-bound)
    // back-substitution + exp-map below; every later pass is requested one pass ahead
    float pX, pY, pZ, pU, pV;
    {
        const int64_t g0 = start + (lane < n ? lane : 0);
        pX = a.x[g0]; pY = a.y[g0]; pZ = a.z[g0]; pU = a.u[g0]; pV = a.v[g0];
    }
    {
        // candidate pose = accepted pose + back-substitution of the previous camera solve
        // (dp = -L^-T (y_r + Y dc)), then the frame constants; wave-uniform, scalar loads
        const int slot = __builtin_amdgcn_readfirstlane(a.obs_slot[f]);
        double pose[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) pose[i] = a.poses[cur][(int64_t)slot * 6 + i];
        double mc = 0.0;
        if (!first) {
            const double* pf = a.pf[cur] + (int64_t)slot * a.PF;
            if (pf[0] != 0.0) {
                double dp[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    const double* yr = pf + 21 + i * K1;
                    double t = yr[K];
#pragma unroll
                    for (int j = 0; j < K; ++j) t += yr[j] * a.dc[j];
                    dp[i] = -t;
                }
#pragma unroll
                for (int i = 5; i >= 0; --i) {
                    double t = dp[i];
#pragma unroll
                    for (int k = i + 1; k < 6; ++k) t -= pf[k * (k + 1) / 2 + i] * dp[k];
                    dp[i] = t * pf[i * (i + 1) / 2 + i];
                }
                const double lam = st->lambda_solve;
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    const double gp = pf[21 + 6 * K1 + i], dCi = pf[21 + 6 * K1 + 6 + i];
                    const double Dii = lam > 0.0 ? lam * clampd1(dCi, a.min_diag, a.max_diag) : 0.0;
                    mc += dp[i] * (Dii * dp[i] - gp);
                    pose[i] += dp[i];
                }
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) if (lane == i) a.poses[es][(int64_t)slot * 6 + i] = pose[i];
        }
        if (lane == 0) a.mc_f[f] = mc;
        double fcr[FC_N0];
        frame_setup<false>(pose, nullptr, fcr);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < FC_N0; ++i) fc[i] = fcr[i];
        }
    }
    wsync();

    d4 acc0 = { 0, 0, 0, 0 }, acc1 = { 0, 0, 0, 0 };
    const int rd_off = (lane >> 5) * CS + ((lane >> 4) & 1) * RS + (lane & 15);
    for (int base = 0; base < n; base += 64) {
        const int c = base + lane;
        const bool valid = c < n;
        const double X = pX, Y = pY, Z = pZ, uo = pU, vo = pV;
        if (base + 64 < n) {                                              // wave-uniform: next pass in flight
            const int cn = base + 64 + lane;
            const int64_t gn = start + (cn < n ? cn : 0);
            pX = a.x[gn]; pY = a.y[gn]; pZ = a.z[gn]; pU = a.u[gn]; pV = a.v[gn];
        }
        double ru, rv, J[2 * D];
        corner_block<MODEL, OF, false, true>(th, fc, X, Y, Z, uo, vo, ru, rv, J, J + D);      // rotation columns in the phi basis
        const double sw = valid ? huber_sqrt_weight(ru * ru + rv * rv, a.huber_delta) : 0.0;
        const int nv = min(64, n - base);
#pragma unroll
        for (int half = 0; half < 64 / GRAM_TILE_CORNERS; ++half) {
            if (half * GRAM_TILE_CORNERS >= nv) break;                    // wave-uniform
            if ((lane / GRAM_TILE_CORNERS) == half) {
                double* row = tile + (lane % GRAM_TILE_CORNERS) * CS;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
#pragma unroll
                    for (int i = 0; i < RS; i += 2) {
                        const double v0 = i < D ? sw * J[h * D + (i < D ? i : 0)] : (i == D ? sw * (h ? rv : ru) : 0.0);
                        const double v1 = (i + 1) < D ? sw * J[h * D + ((i + 1) < D ? (i + 1) : 0)] : ((i + 1) == D ? sw * (h ? rv : ru) : 0.0);
                        *reinterpret_cast<double2*>(row + h * RS + i) = make_double2(v0, v1);
                    }
                }
            }
            wsync();
            const int npairs = (min(GRAM_TILE_CORNERS, nv - half * GRAM_TILE_CORNERS) + 1) >> 1;
            const double* rd = tile + rd_off;
            int m = 0;
            for (; m + 1 < npairs; m += 2) {
                const double p = rd[(2 * m) * CS];
                const double q = rd[(2 * m + 2) * CS];
                acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(p, p, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(q, q, acc1, 0, 0, 0);
            }
            if (m < npairs) {
                const double p = rd[(2 * m) * CS];
                acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(p, p, acc0, 0, 0, 0);
            }
            wsync();
        }
    }
    // Gram -> LDS (aliases the tile), then the compact record.  Columns: camera 0..K-1, pose K..K+5, r = D.
    double* G = tile;
    {
        const d4 acc = acc0 + acc1;
        const int gi = lane >> 4, gj = lane & 15;
#pragma unroll
        for (int v = 0; v < 4; ++v) G[(gi + 4 * v) * 16 + gj] = acc[v];
    }
    wsync();
    double* rec = a.praw[es] + (int64_t)f * a.PRAW;
    if (lane < 21) {
        int i = 0, r = lane;
        while (r > i) { r -= i + 1; ++i; }          // lane -> (i, r) of the packed lower triangle
        rec[lane] = G[(K + i) * 16 + (K + r)];
    }
    for (int e = lane; e < 6 * K1; e += 64) {
        const int i = e / K1, j = e - i * K1;
        rec[21 + e] = G[(K + i) * 16 + (j < K ? j : D)];
    }
    for (int e = lane; e < K1 * K1; e += 64) {
        const int i = e / K1, j = e - i * K1;
        rec[21 + 6 * K1 + e] = G[(i < K ? i : D) * 16 + (j < K ? j : D)];
    }
    if (lane == 0) a.cost_f[f] = G[D * 16 + D];
    if (lane < 9) rec[praw_jl_off(K) + lane] = fc[FC_A + lane];      // the frame's left Jacobian: the elimination maps phi -> rvec with it
}

template <int MODEL, bool OF>
static hipError_t launch_gram1_t(const FusedArgs& a, hipStream_t s) {
    constexpr int WS = FC_N0P + GRAM_TILE_CORNERS * 34;
    const size_t lds = sizeof(double) * WS * WAVES_PER_BLOCK;
    static DynLdsGuard lds_guard;
    if (hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(&k_gram1<MODEL, OF>), lds, lds_guard); e != hipSuccess) return e;
    hipLaunchKernelGGL((k_gram1<MODEL, OF>), dim3((a.n_obs + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK), dim3(256), lds, s, a);
    return hipGetLastError();
}
hipError_t launch_gram1(int model, bool one_focal, const FusedArgs& a, hipStream_t s) {
    return dispatch_model_focal(model, one_focal, hipErrorInvalidValue, [&](auto m, auto of) { return launch_gram1_t<decltype(m)::value, decltype(of)::value>(a, s); });
}

// ---------------------------------------------------------------------------------------------
// k_schur1m: the elimination with FOUR frames per wavefront (16 lanes each), one pass per wavefront: the grid covers all frames
// (n_pw = 4 ceil(n_obs / 16)).
// ---------------------------------------------------------------------------------------------
constexpr int SCHUR1M_WAVES = 8;          // 32 frames per workgroup: a quarter of the partial sums k_head / k_reduce1 have to add up
template <int K>
__global__ __launch_bounds__(64 * SCHUR1M_WAVES) void k_schur1m(const FusedArgs a) {
    constexpr int K1 = K + 1, NA = K1 * K1;
    constexpr int NQ = (NA + 15) / 16;                    // A / Y^T Y entries per lane
    constexpr int REC = 21 + 6 * K1 + NA + 9;             // C (21) | [B|g] (6 x K1) | A (K1 x K1) | J_l (9)
    constexpr int GS = (REC + 6 * K1 + 1) & ~1;           // per frame in LDS: record | Y (6 x K1); later the frame's sums
    constexpr int NF = 4 * SCHUR1M_WAVES;                 // frames per workgroup
    static_assert(2 * NA + 2 <= GS, "a frame's sums reuse its record row");
    __shared__ double smem[NF * GS];
    const DevState* st = a.st;
    if (st->done) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int grp = lane >> 4, gl = lane & 15;
    const int f = (blockIdx.x * SCHUR1M_WAVES + wave) * 4 + grp;
    const bool active = f < a.n_obs;
    double* R = smem + (wave * 4 + grp) * GS;
    double* Ym = R + REC;
    const int set = schur_set(st);
    const double lambda = schur_lambda(st);
    double accA[NQ], accY[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) { accA[q] = 0.0; accY[q] = 0.0; }
    double mcv = 0.0;
    if (active) {
        const double* rec = a.praw[set] + (int64_t)f * a.PRAW;
        for (int e = gl; e < REC; e += 16) R[e] = rec[e];
        if (gl == 0) mcv = a.mc_f[f];
    }
    const int slot = active ? a.obs_slot[f] : 0;
    wsync();
    const bool ok = eliminate_frame<K, 16>(R, Ym, gl, active, lambda, a.min_diag, a.max_diag,
                                          a.pf[set] + (int64_t)slot * a.PF, a.PF, accA, accY);
    // the frames of the workgroup combine in LDS (fixed order), one flush per workgroup; a frame's sums reuse its row
    wsync();
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int e = gl + 16 * q;
        if (e < NA) { R[e] = accA[q]; R[NA + e] = accY[q]; }
    }
    if (gl == 0) { R[2 * NA] = mcv; R[2 * NA + 1] = (active && !ok) ? 1.0 : 0.0; }
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * NA + 2; e += 64 * SCHUR1M_WAVES) {
        double t = 0.0;
#pragma unroll
        for (int g = 0; g < NF; ++g) t += smem[g * GS + e];
        a.partial[(int64_t)blockIdx.x * (2 * NA + 2) + e] = t;
    }
}
hipError_t launch_schur1m(FusedArgs& a, hipStream_t s) {
    const dim3 grid((a.n_obs + 4 * SCHUR1M_WAVES - 1) / (4 * SCHUR1M_WAVES)), blk(64 * SCHUR1M_WAVES);
    a.n_part = (int32_t)grid.x;
    if (grid.x == 0) return hipSuccess;
    switch (a.K) {
        case 4: hipLaunchKernelGGL(k_schur1m<4>, grid, blk, 0, s, a); break;
        case 5: hipLaunchKernelGGL(k_schur1m<5>, grid, blk, 0, s, a); break;
        case 6: hipLaunchKernelGGL(k_schur1m<6>, grid, blk, 0, s, a); break;
        case 7: hipLaunchKernelGGL(k_schur1m<7>, grid, blk, 0, s, a); break;
        case 8: hipLaunchKernelGGL(k_schur1m<8>, grid, blk, 0, s, a); break;
        case 9: hipLaunchKernelGGL(k_schur1m<9>, grid, blk, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace ccal

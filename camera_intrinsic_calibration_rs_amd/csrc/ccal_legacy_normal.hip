// Second library only (libccal_hip_legacy.so, -DCCAL_LEGACY_KERNELS): the matrix-core Gram of the general (multi-camera) loop,
// superseded by the register Gram kernels for every model (CCAL_GENERAL_GRAM=mfma selects it).  It leaves 16 x 16 tiles or
// 32-stride blocks, which the table-driven k_schur<false, 4> (ccal_kernels_normal.hip) eliminates.  The parity tests keep the pair
// as the independent second implementation they hold the product kernels against.
#include "ccal_device.hpp"
#include "ccal_fused.hpp"
#include "ccal_gram_common.hpp"

namespace ccal {

struct GramArgs {
    KArgs k;
    const int64_t* goff;
    double* G;
    double* cost_o;
    // device-resident loop: st != NULL evaluates the set the state prescribes (eval_set: the starting point in the first
    // group, the candidate afterwards; index 0 = this set, 1 = the second one); finished solves and re-elimination
    // groups make the launch empty
    const DevState* st;
    const double* intr2; const double* poses2; const double* extr2; double* G2; double* cost_o2;
};

// ---------------------------------------------------------------------------------------------
// k_gram: one wavefront per observation frame.  Every lane evaluates one corner's two weighted
// rows sqrt(w) [J | r] (NC = D + 1 columns), the wave stages them in LDS as a [rows][16 T] image and
// v_mfma_f64_16x16x4_f64 accumulates G += rows^T rows, 4 rows (2 corners) per instruction: the
// lane that feeds A[i][k] also feeds B[k][j] (same register), so a Gram tile costs one ds_read_b64
// and one MFMA.  T = 1 (NC <= 16: every single-camera model) or 2 (other-camera blocks, NC <= 22).
// ---------------------------------------------------------------------------------------------
template <int MODEL, bool OF, bool OTHER>
__global__ __launch_bounds__(256) void k_gram(const GramArgs ga) {
    const KArgs& a = ga.k;
    if (ga.st && (ga.st->done || ga.st->redo)) return;
    const bool second = ga.st && eval_set(ga.st) == 1;
    const double* p_intr = second ? ga.intr2 : a.intr;
    const double* p_poses = second ? ga.poses2 : a.poses;
    const double* p_extr = second ? ga.extr2 : a.extr;
    double* p_G = second ? ga.G2 : ga.G;
    double* p_cost = second ? ga.cost_o2 : ga.cost_o;
    constexpr int D = block_dim(MODEL, OF, OTHER);
    // Other-camera blocks: d r / d tvec_0_b = (d r / d tvec_c_0) R_c0, so those three columns are linear combinations
    // of three others with per-camera constant coefficients.  When the remaining D - 3 + 1 columns fit ONE 16 x 16
    // matrix-core tile (UCM / EUCM rigs) the Gram is built without them (one MFMA per corner pair instead of
    // three) and k_schur expands it with R_c0, which is stored behind the tile.
    constexpr bool CMP = gram_compact(MODEL, OF, OTHER);
    constexpr int PE = D - (OTHER ? 12 : 6);
    constexpr int NC = CMP ? D - 2 : D + 1;   // staged columns (the last one is the residual)
    constexpr int RC = NC - 1;                // index of the residual column
    constexpr int T = NC <= 16 ? 1 : 2;
    constexpr int RS = T == 1 ? 16 : 24;      // doubles per staged row
    constexpr int CS = 2 * RS + 2;            // doubles per corner (two rows + pad)
    constexpr int NCP = 16 * T;
    constexpr int FCN = OTHER ? FC_SIZE : FC_N0P;
    constexpr int WS = FCN + GRAM_TILE_CORNERS * CS;   // rows are staged 32 corners at a time (LDS -> occupancy)
    extern __shared__ double smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int widx = blockIdx.x * WAVES_PER_BLOCK + wave;
    if (widx >= a.n_list) return;
    double* fc = smem + wave * WS;
    double* tile = fc + FCN;

    const int o = __builtin_amdgcn_readfirstlane(a.list[widx]);
    const int slot = __builtin_amdgcn_readfirstlane(a.obs_slot[o]);
    const int64_t start = a.obs_off[o];
    const int n = (int)(a.obs_off[o + 1] - start);
    const double* th_g = p_intr + a.cam * CCAL_PMAX;
    double th[th_len<MODEL>()];
    load_theta<MODEL, OF>(th_g, a.rt, th);
    {
        double pose[6], ex[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) pose[i] = p_poses[(int64_t)slot * 6 + i];
        if constexpr (OTHER) {
#pragma unroll
            for (int i = 0; i < 6; ++i) ex[i] = p_extr[a.cam * 6 + i];
        }
        double fcr[OTHER ? FC_SIZE : FC_N0];
        frame_setup<OTHER>(pose, ex, fcr);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < (OTHER ? FC_SIZE : FC_N0); ++i) fc[i] = fcr[i];
        }
    }
    wsync();

    d4 acc00a = { 0, 0, 0, 0 }, acc00b = { 0, 0, 0, 0 }, acc01 = { 0, 0, 0, 0 }, acc11 = { 0, 0, 0, 0 };
    // read position of this lane inside a corner pair: corner (lane >> 5), row (lane >> 4) & 1, column lane & 15
    const int rd_off = (lane >> 5) * CS + ((lane >> 4) & 1) * RS + (lane & 15);
    const bool hi_valid = (lane & 15) < (RS - 16);          // T == 2: columns 16..RS-1 exist, the rest are zero

    for (int base = 0; base < n; base += 64) {
        const int c = base + lane;
        const bool valid = c < n;
        const int64_t g = start + (valid ? c : 0);
        const double X = a.x[g], Y = a.y[g], Z = a.z[g], uo = a.u[g], vo = a.v[g];
        double ru, rv, J[2 * D];
        corner_block<MODEL, OF, OTHER>(th, fc, X, Y, Z, uo, vo, ru, rv, J, J + D);
        // Huber corrector: both rows scaled by sqrt(rho'); invalid lanes contribute zero rows
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
                        // staged column -> Jacobian column (compact form skips tvec_0_b: PE+3 .. PE+5)
                        const int s0 = (CMP && i >= PE + 3) ? i + 3 : i, s1 = (CMP && i + 1 >= PE + 3) ? i + 4 : i + 1;
                        const double v0 = i < RC ? sw * J[h * D + (i < RC ? s0 : 0)] : (i == RC ? sw * (h ? rv : ru) : 0.0);
                        const double v1 = (i + 1) < RC ? sw * J[h * D + ((i + 1) < RC ? s1 : 0)] : ((i + 1) == RC ? sw * (h ? rv : ru) : 0.0);
                        *reinterpret_cast<double2*>(row + h * RS + i) = make_double2(v0, v1);
                    }
                }
            }
            wsync();
            const int npairs = (min(GRAM_TILE_CORNERS, nv - half * GRAM_TILE_CORNERS) + 1) >> 1;
            const double* rd = tile + rd_off;
            if constexpr (T == 1) {
                int m = 0;
                for (; m + 1 < npairs; m += 2) {
                    const double p = rd[(2 * m) * CS];
                    const double q = rd[(2 * m + 2) * CS];
                    acc00a = __builtin_amdgcn_mfma_f64_16x16x4f64(p, p, acc00a, 0, 0, 0);
                    acc00b = __builtin_amdgcn_mfma_f64_16x16x4f64(q, q, acc00b, 0, 0, 0);
                }
                if (m < npairs) {
                    const double p = rd[(2 * m) * CS];
                    acc00a = __builtin_amdgcn_mfma_f64_16x16x4f64(p, p, acc00a, 0, 0, 0);
                }
            } else {
                for (int m = 0; m < npairs; ++m) {
                    const double p = rd[(2 * m) * CS];
                    const double q = hi_valid ? rd[(2 * m) * CS + 16] : 0.0;
                    acc00a = __builtin_amdgcn_mfma_f64_16x16x4f64(p, p, acc00a, 0, 0, 0);
                    acc01 = __builtin_amdgcn_mfma_f64_16x16x4f64(p, q, acc01, 0, 0, 0);
                    acc11 = __builtin_amdgcn_mfma_f64_16x16x4f64(q, q, acc11, 0, 0, 0);
                }
            }
            wsync();
        }
    }

    // C/D layout of v_mfma_f64_16x16x4_f64: lane l, register v holds D[(l >> 4) + 4 v][l & 15]
    double* Go = p_G + ga.goff[o];
    const int gi = lane >> 4, gj = lane & 15;
    if constexpr (CMP) {
        // compact tile -> the block-upper-triangular 32-stride layout k_schur reads (rows 0..15 x all columns, rows 16.. x
        // columns 16..), with the tvec_0_b rows / columns restored: column a = sum_m R_c0[m][a] tvec_c_0[m].
        // Three branch-free passes: the tile's own entries straight from the accumulator registers, the 3 x 16 restored
        // rows (+ their mirror), the 3 x 3 restored block.
        const d4 acc = acc00a + acc00b;
        constexpr int TC = PE + 6;                          // first tvec_c_0 column of the compact tile
        wsync();
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int ci = gi + 4 * v, cj = gj;
            tile[ci * 17 + cj] = acc[v];
            const int i = ci < PE + 3 ? ci : ci + 3, j = cj < PE + 3 ? cj : cj + 3;     // compact -> virtual column
            if (!(i >= 16 && j < 16)) Go[i * 32 + j] = acc[v];                          // lower-left tile is never read
            if (ci == RC && cj == RC) p_cost[o] = acc[v];
        }
        wsync();
        const double* R1 = fc + FC_R1;
        if (lane < 48) {
            const int aa = lane >> 4, cj = lane & 15;
            double val = 0.0;
#pragma unroll
            for (int m = 0; m < 3; ++m) val += R1[m * 3 + aa] * tile[(TC + m) * 17 + cj];
            const int i = PE + 3 + aa, j = cj < PE + 3 ? cj : cj + 3;
            Go[i * 32 + j] = val;
            if (j < 16) Go[j * 32 + i] = val;
        } else if (lane < 57) {
            const int aa = (lane - 48) / 3, ab = (lane - 48) % 3;
            double val = 0.0;
#pragma unroll
            for (int m = 0; m < 3; ++m)
#pragma unroll
                for (int n2 = 0; n2 < 3; ++n2) val += R1[m * 3 + aa] * R1[n2 * 3 + ab] * tile[(TC + m) * 17 + TC + n2];
            Go[(PE + 3 + aa) * 32 + PE + 3 + ab] = val;
        }
    } else if constexpr (T == 1) {
        const d4 acc = acc00a + acc00b;
#pragma unroll
        for (int v = 0; v < 4; ++v) Go[(gi + 4 * v) * NCP + gj] = acc[v];
        if (gi + 4 * (RC / 4) == RC && gj == RC) p_cost[o] = acc[RC / 4];
    } else {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            Go[(gi + 4 * v) * NCP + gj] = acc00a[v];
            Go[(gi + 4 * v) * NCP + 16 + gj] = acc01[v];
            Go[(16 + gi + 4 * v) * NCP + 16 + gj] = acc11[v];
        }
        constexpr int dl = RC - 16;  // residual column lives in tile (1,1)
        if (gi + 4 * (dl / 4) == dl && gj == dl) p_cost[o] = acc11[dl / 4];
    }
}

template <int MODEL, bool OF, bool OTHER>
static hipError_t launch_gram_t(const GramArgs& ga, hipStream_t s) {
    constexpr int D = block_dim(MODEL, OF, OTHER);
    constexpr int T = (gram_compact(MODEL, OF, OTHER) ? D - 2 : D + 1) <= 16 ? 1 : 2;
    constexpr int RS = T == 1 ? 16 : 24;
    constexpr int WS = (OTHER ? FC_SIZE : FC_N0P) + GRAM_TILE_CORNERS * (2 * RS + 2);
    const size_t lds = sizeof(double) * WS * WAVES_PER_BLOCK;
    const int blocks = (ga.k.n_list + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    if (blocks == 0) return hipSuccess;
    static DynLdsGuard lds_guard;
    if (hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(&k_gram<MODEL, OF, OTHER>), lds, lds_guard); e != hipSuccess) return e;
    hipLaunchKernelGGL((k_gram<MODEL, OF, OTHER>), dim3(blocks), dim3(256), lds, s, ga);
    return hipGetLastError();
}

// what both launchers share: the corners, camera `cam`'s list of observation frames, the tiles' offsets
static GramArgs gram_args(const ccal_problem* p, int cam) {
    GramArgs ga = {};
    KArgs& a = ga.k;
    a.x = p->d_x; a.y = p->d_y; a.z = p->d_z; a.u = p->d_u; a.v = p->d_v;
    a.obs_off = p->d_obs_off; a.obs_slot = p->d_obs_slot; a.joff = p->d_joff;
    a.list = p->cams[cam].d_obs; a.n_list = (int32_t)p->cams[cam].obs.size(); a.cam = cam;
    a.huber_delta = p->huber_delta; a.rt = model_rt(p->ctx);
    ga.goff = p->nws->d_goff;
    return ga;
}
static hipError_t launch_gram_m(const ccal_problem* p, int cam, const GramArgs& ga, hipStream_t s) {
    return dispatch_model_focal_other(p->cams[cam].model, p->one_focal, cam > 0, hipErrorInvalidValue, [&](auto m, auto of, auto other) {
        return launch_gram_t<decltype(m)::value, decltype(of)::value, decltype(other)::value>(ga, s);
    });
}
// host-driven build: the current or the candidate parameters into G[gbuf]
hipError_t launch_gram(const ccal_problem* p, int cam, bool cand, int gbuf, hipStream_t s) {
    const NormalWs* w = p->nws;
    GramArgs ga = gram_args(p, cam);
    ga.k.intr = cand ? p->d_intr_c : p->d_intr; ga.k.poses = cand ? p->d_poses_c : p->d_poses; ga.k.extr = cand ? p->d_extr_c : p->d_extr;
    ga.G = w->G[gbuf]; ga.cost_o = w->cost_o[gbuf];
    return launch_gram_m(p, cam, ga, s);
}
// device-resident loop (what launch_gram_dev calls when the workspace was planned without the register Gram):
// set 0 = (p->d_*, G[w->cur]), set 1 = (p->d_*_c, G[w->cur ^ 1])
hipError_t launch_gram_dev_mfma(const ccal_problem* p, int cam, const DevState* st, hipStream_t s) {
    const NormalWs* w = p->nws;
    GramArgs ga = gram_args(p, cam);
    ga.k.intr = p->d_intr; ga.k.poses = p->d_poses; ga.k.extr = p->d_extr;
    ga.intr2 = p->d_intr_c; ga.poses2 = p->d_poses_c; ga.extr2 = p->d_extr_c;
    ga.G = w->G[w->cur]; ga.cost_o = w->cost_o[w->cur]; ga.G2 = w->G[w->cur ^ 1]; ga.cost_o2 = w->cost_o[w->cur ^ 1];
    ga.st = st;
    return launch_gram_m(p, cam, ga, s);
}

}  // namespace ccal

// Single-camera fast path of the optimizer: the whole Gauss-Newton / LM iteration is device-resident,
// the host only enqueues kernels and watches a status word in pinned memory.
//
//   k_unpack1       the starting point of a solve (state, column table, intrinsics in the argument block; poses from pinned host memory)
//   k_gram1v        LPF lanes per frame, the whole upper triangle of [J | r]^T W [J | r] in registers, the frame's pose block
//                   eliminated in the kernel's tail (gram_fused_tail): one row of partial sums per wavefront.  UCM / EUCM / KB4
//                   below 2 000 frames (k_gram2, ccal_kernels_gram2.hip, from there on and for OPENCV5)
//   k_gram1v<ITER>  the same with the PREVIOUS launch's rows summed, the decision taken and the camera system solved in front of
//                   the evaluation: a whole optimizer step in one launch (session sizes)
//   k_gram1v_batch  that launch for a whole batch of problems (ccal_solve_batch: blockIdx.y = problem, lockstep)
//   k_reduce1       fixed-order sum over the rows -> red (the all-reduce buffer of sharded solves)
//   k_head          one wavefront: accept / reject / convergence tests (tiny-solver's rules or the Ceres-style trust region),
//                   K x K solve, candidate intrinsics, status to pinned host memory; in-process transport: adds the ranks' sums
// Every kernel here is in the product library.  The superseded matrix-core Gram (k_gram1) and the separate elimination launch
// (k_schur1m) are in ccal_legacy_fused.hip, which only the second library contains.
// Same arithmetic and decision sequence as the general loop in ccal_solver.hip (multi-camera problems);
// parity tests cover both.
#include <algorithm>
#include <cstdlib>

#include "ccal_device.hpp"
#include "ccal_fused.hpp"
#include "ccal_gram_common.hpp"
#include "ccal_head.hpp"
#include "ccal_devopt.hpp"

namespace ccal {

// ---------------------------------------------------------------------------------------------
// k_unpack1: the starting point of a solve in ONE launch.  Optimizer state, column table and intrinsics ride in the kernel's
// argument block (round 4; they were a staging copy the kernel then waited for), the poses are read where the caller left them:
// pinned host memory for session-sized problems (zero-copy: no H2D operation at all), a staged device copy for large ones.
// Both parameter sets start from the caller's values; slots without observations never change.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_unpack1(const UnpackArgs a) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, nt = (int64_t)gridDim.x * 256;
    // ccal_solve_dev: the starting point already sits in set 0 on the device - only mirror it into set 1
    const double* poses = a.poses_on_device ? a.poses0 : a.poses_src;
    for (int64_t e = t; e < a.np6; e += nt) { const double v = poses[e]; if (!a.poses_on_device) a.poses0[e] = v; a.poses1[e] = v; }
    if (blockIdx.x == 0) {
        constexpr int NS = (int)(sizeof(DevState) / sizeof(double)), NC1 = (int)(sizeof(ColInfo) / sizeof(double));
        for (int e = threadIdx.x; e < CCAL_PMAX; e += 256) {
            const double v = a.poses_on_device ? a.intr0[e] : a.intr_h[e];
            if (!a.poses_on_device) a.intr0[e] = v;
            a.intr1[e] = v;
        }
        for (int e = threadIdx.x; e < NS; e += 256) reinterpret_cast<double*>(a.st)[e] = reinterpret_cast<const double*>(&a.st0)[e];
        for (int e = threadIdx.x; e < a.n_cols * NC1; e += 256) reinterpret_cast<double*>(a.cols)[e] = reinterpret_cast<const double*>(a.col0)[e];
    }
}
hipError_t launch_unpack1(const UnpackArgs& a, hipStream_t s) {
    const int blocks = (int)std::min<int64_t>(std::max<int64_t>((a.np6 + 255) / 256, 1), 1024);
    hipLaunchKernelGGL(k_unpack1, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// k_gram1v: the same per-frame record as k_gram1 (the matrix-core kernel of round 1, ccal_legacy_fused.hip), without the LDS
// transposition the matrix cores need.
// Measured (profiles/r01, ablations in DESIGN.md): staging sqrt(w)[J|r] rows through LDS in MFMA operand
// order costs ~45 us of k_gram1's 69 us at 10 000 frames, and f64 MFMA shares the FP64 datapath with the
// VALU on gfx950 (no overlap).  Here 16 lanes own one frame (4 frames per wavefront; 144 corners = 9 x 16,
// no idle lanes), every lane keeps the upper triangle of [J|r]^T W [J|r] in registers (structural zeros of
// the intrinsic columns skipped at compile time) and the 16 partial Grams of a frame meet once in LDS.
// ---------------------------------------------------------------------------------------------
// Where each accumulated triangle entry goes inside the compact per-frame record
// C (21) | [B|g] (6 x K1) | A (K1 x K1, both halves), worked out at compile time: dst | mirror << 16 (0xffff = none).
template <int K, bool GEN = false>
struct RecMap {
    static constexpr int D = K + 6, NC = D + 1, K1 = K + 1;
    static constexpr int N = NC * (NC + 1) / 2;
    uint32_t d[N];
    constexpr RecMap() : d{} {
        int r = 0;
        for (int i = 0; i < NC; ++i)
            for (int j = i; j < NC; ++j) {
                const bool ip = i >= K && i < D, jp = j >= K && j < D;      // pose columns
                const int ci = i < K ? i : K, cj = j < K ? j : K;           // camera-block index (r -> K)
                uint32_t a = 0, b = 0xffff;
                if (!GEN) {
                    if (ip && jp) a = (j - K) * (j - K + 1) / 2 + (i - K);
                    else if (!ip && jp) a = 21 + (j - K) * K1 + ci;             // i camera, j pose
                    else if (ip && !jp) a = 21 + (i - K) * K1 + K;              // i pose, j = r
                    else { a = 21 + 6 * K1 + ci * K1 + cj; b = 21 + 6 * K1 + cj * K1 + ci; }
                } else {                                                        // GEN record (ccal_fused.hpp)
                    if (ip && jp) { a = (i - K) * 6 + (j - K); if (i != j) b = (j - K) * 6 + (i - K); }
                    else if (!ip && jp) a = 36 + ci * 6 + (j - K);
                    else if (ip && !jp) a = 36 + K * 6 + (i - K);
                    else a = gen_a_off(K) + cj * (cj + 1) / 2 + ci;            // packed lower triangle (ci <= cj)
                }
                d[r++] = a | (b << 16);
            }
    }
};
template <int K, bool GEN = false> __device__ const RecMap<K, GEN> g_recmap = RecMap<K, GEN>();

// doubles of LDS per wavefront of k_gram1v at lpf lanes per frame: the frames' constants | the reduction buffer.
// The kernel asserts its own layout against it, the launchers size by it.
template <int MODEL, bool OF>
constexpr int gram1_wave_lds(int lpf) {
    constexpr int NC = block_dim(MODEL, OF, false) + 1, NE = NC * (NC + 1) / 2;
    constexpr int LS = ((NE + 1) / 2) | 1;
    return (64 / lpf) * FC_N0P + 64 * LS;
}
// structural zeros of the block Jacobian rows (u row: no fy, cy; v row: no fx, cx); f feeds both rows
template <bool OF> __device__ constexpr bool nz_u(int i) { return OF ? (i != 2) : (i != 1 && i != 3); }
template <bool OF> __device__ constexpr bool nz_v(int i) { return OF ? (i != 1) : (i != 0 && i != 2); }

// LPF = lanes per frame (16, 32 or 64): small problems spread a frame over more lanes so that the chip still fills.
// GEN: one camera's blocks of the general (multi-camera) loop - the frames are those of a.list, the slot pose is read as it
// stands (k_backsub has formed it) and composed with the camera's extrinsics (frame_setup_composed): the six pose columns
// are those of the COMPOSED pose, in the phi basis, for every camera; the record goes to the observation frame's place in
// the Gram buffer (a.rec_off) together with the blocks of the matrix that expands it to the block's reference columns.
// ITER (single-camera loop, session sizes; IterArgs in ccal_fused.hpp): a group in ONE launch - four wavefronts per workgroup;
// in front of the evaluation every workgroup sums the previous launch's rows (reduce_partial_rows: k_head's order), its first
// wavefront decides and solves the camera system (head_wave), and the evaluation takes state, camera step and candidate
// intrinsics from LDS; behind it the four wavefronts' rows of partial sums are added in LDS: one row per workgroup.
// What changes from one single-launch group of a solve to the next - in the argument block (IterArgs) when a launch serves ONE
// problem, derived from the launch number when it serves a whole batch (k_gram1v_batch: the table of argument blocks is written once).
struct IterDyn { int32_t seq, skip_head, fold; const DevState* st_in; DevState* st_out; const double* partial_in; double* partial_out; };
template <int MODEL, bool OF, int LPF, bool GEN, bool ITER>
__device__ __forceinline__ void gram1v_body(const FusedArgs& a, const IterDyn& dy) {
    static_assert(!(ITER && GEN), "single-launch groups: single-camera loop only");
    constexpr int WPB = ITER ? 4 : CCAL_GRAMV_WPB;
    constexpr int G = 64 / LPF;                     // frames per wavefront
    constexpr int D = block_dim(MODEL, OF, false);
    constexpr int K = D - 6, K1 = K + 1;
    constexpr int NC = D + 1;                       // columns of [J | r]
    constexpr int NE = NC * (NC + 1) / 2;           // upper triangle
    constexpr int HALF = (NE + 1) / 2;              // entries reduced per LDS round
    constexpr int LS = HALF | 1;                    // odd row stride (doubles): conflict-free column sums
    constexpr int WSL = G * FC_N0P + 64 * LS;           // per wave: G frames' constants | reduction buffer
    static_assert(WSL == gram1_wave_lds<MODEL, OF>(LPF),"the launchers size the LDS by gram1_wave_lds");
    constexpr int NQ = (G * HALF + 63) / 64;        // (frame, entry) sums per lane and round
    extern __shared__ double smem[];
#ifdef CCAL_STAMPS          // diagnostic build (tools/stamps_g1v.py): the phases of every wavefront, 8 stamps per wavefront in the per-frame scratch
    long long ts[12] = {};
    ts[0] = wall_clock64();
#define G1V_STAMP(i) ts[i] = wall_clock64()
#else
#define G1V_STAMP(i)
#endif
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // LPF need not divide 64 (12 lanes x 5 frames, 6 x 10): the lanes beyond G * LPF idle along with group G - 1
    const bool lane_ok = lane < G * LPF;
    const int grp = lane_ok ? lane / LPF : G - 1, gl = lane % LPF;
    const int f = (blockIdx.x * WPB + wave) * G + grp;
    const bool active = lane_ok && f < a.n_obs;
    const int fa_ = GEN ? a.list[active ? f : 0] : (active ? f : 0);      // observation frame (GEN: the camera's list)
    // ITER: everything the prologue below reads from global memory is requested in FRONT of the decision - the frame's offsets
    // and slot before the sum over the previous launch's rows, pose / elimination record / first corner rows (both parameter
    // sets: the decision picks one) behind that sum's loads and before its workgroup barriers: the prologue's two dependent round
    // trips run beside the decision instead of behind it (stamps, 625 frames: prologue 3.2 -> 2.1 us)
    constexpr int PFLEN = 33 + 6 * (D - 6 + 1);                // the slot's elimination record: L (21) | Y (6 x K1) | g_p (6) | diag C (6)
    constexpr int NPFQ = ITER ? (PFLEN + LPF - 1) / LPF : 1;
    int64_t start_p = 0; int n_p = 0, slot_p = 0;
    float pX = 0.f, pY = 0.f, pZ = 0.f, pU = 0.f, pV = 0.f;
    double pose_p[2][ITER ? 6 : 1], pf_p[2][NPFQ];
    if constexpr (ITER) {
        start_p = a.obs_off[fa_];
        n_p = active ? (int)(a.obs_off[fa_ + 1] - start_p) : 0;
        slot_p = a.obs_slot[fa_];
    }
    bool fold_first = false;                        // ITER: this launch is also the solve's k_unpack1 (IterArgs::fold)
    if constexpr (ITER) fold_first = dy.skip_head != 0 && dy.fold != 0;
    auto iter_prefetch2 = [&]() {
      if constexpr (ITER) {
        const int64_t g0 = start_p + (gl < n_p ? gl : 0);
        pX = a.x[g0]; pY = a.y[g0]; pZ = a.z[g0]; pU = a.u[g0]; pV = a.v[g0];
        // (fold: the starting pose from where the caller left it - pinned host memory, or set 0 for device-resident solves)
        const double* ps0 = fold_first ? (a.it.poses_on_device ? a.poses[0] : a.it.poses_src) : a.poses[0];
        const double* ps1 = fold_first ? ps0 : a.poses[1];
#pragma unroll
        for (int i = 0; i < 6; ++i) { pose_p[0][i] = ps0[(int64_t)slot_p * 6 + i]; pose_p[1][i] = ps1[(int64_t)slot_p * 6 + i]; }
#pragma unroll
        for (int q = 0; q < NPFQ; ++q) {
            const int e = min(gl + LPF * q, PFLEN - 1);
            pf_p[0][q] = a.pf[0][(int64_t)slot_p * a.PF + e]; pf_p[1][q] = a.pf[1][(int64_t)slot_p * a.PF + e];
        }
      }
    };
    // what the evaluation needs of the optimizer state, in registers (the single-launch form decides in this kernel: LDS; else global)
    struct { int done, redo, cur, first, method; double lambda_solve, lam_schur; } g;
    constexpr int PROW = ITER ? iter_row_len(D - 6) : 1;       // ITER: a workgroup's row of partial sums, symmetric blocks packed
    __shared__ double it_rows[ITER ? 4 : 1][ITER ? fused_red_size(D - 6) : 1];
    __shared__ typename std::conditional<ITER, HeadShared, int>::type hsh;
    bool from_lds = false;                          // ITER, not the first launch: state, camera step and candidate are in hsh
    if constexpr (ITER) {
        const IterArgs& it = a.it;
        if (!dy.skip_head) {
            // (the rows are summed also for a solve that has finished: asking first would put a memory round trip in front of every group's loads)
            HeadIO io;
            io.st_in = dy.st_in; io.st_out = dy.st_out; io.hs = it.hs; io.red_g = nullptr; io.cols = it.cols;
            io.intr[0] = a.intr[0]; io.intr[1] = a.intr[1]; io.dc = it.dc_out; io.K = D - 6; io.seq = dy.seq;
            io.min_diag = a.min_diag; io.max_diag = a.max_diag; io.publish_all = it.publish_all;
            HeadPre hpre = {};
            if (threadIdx.x < 64) hpre = head_prefetch(io, (int)threadIdx.x);
            __shared__ double shr[4][(PROW + 63) / 64][64];
            double vsum[(PROW + 63) / 64][4];
            iter_reduce_load<D - 6>(dy.partial_in, it.n_part_in, vsum);
            iter_prefetch2();
            iter_reduce_combine<D - 6>(vsum, hsh.red, shr);
            G1V_STAMP(7);                                   // the previous launch's rows are summed
            const bool writer = blockIdx.x == 0;
            if (threadIdx.x < 64) head_wave(io, hsh, (int)threadIdx.x, writer, hpre);
            __syncthreads();
            G1V_STAMP(8);                                   // decided, camera system solved
            head_finish(io, hsh, it.result_host, a.poses[0], a.poses[1], it.np6, writer, it.result_poses, it.done_cnt);
            G1V_STAMP(9);
            from_lds = true;
            const DevState& S = hsh.S0;
            g.done = S.done; g.redo = S.redo; g.cur = S.cur; g.first = S.first; g.method = S.method;
            g.lambda_solve = S.lambda_solve; g.lam_schur = schur_lambda(&S);
        } else if (fold_first) {
            iter_prefetch2();
            // the solve's first launch AND its k_unpack1: state, columns and intrinsics from the argument block
            constexpr int NS = (int)(sizeof(DevState) / sizeof(double)), NC1 = (int)(sizeof(ColInfo) / sizeof(double));
            if (threadIdx.x < CCAL_PMAX) hsh.cand[threadIdx.x] = it.poses_on_device ? a.intr[0][threadIdx.x] : reinterpret_cast<const double*>(it.intr_h)[threadIdx.x];
            if (blockIdx.x == 0 && threadIdx.x < 64) {
                for (int e = threadIdx.x; e < NS; e += 64) reinterpret_cast<double*>(dy.st_out)[e] = reinterpret_cast<const double*>(&it.st0)[e];
                for (int e = threadIdx.x; e < it.n_cols * NC1; e += 64) reinterpret_cast<double*>(it.cols_out)[e] = reinterpret_cast<const double*>(it.col0)[e];
                if (threadIdx.x < CCAL_PMAX) {
                    const double v = it.poses_on_device ? a.intr[0][threadIdx.x] : reinterpret_cast<const double*>(it.intr_h)[threadIdx.x];
                    if (!it.poses_on_device) a.intr[0][threadIdx.x] = v;
                    a.intr[1][threadIdx.x] = v;
                }
                if (threadIdx.x == 0) it.hs->word = status_word(dy.seq, 0, 0);
            }
            __syncthreads();
            from_lds = true;                       // (the intrinsics: hsh.cand; the camera step is not read in a first evaluation)
            const DevState& S = it.st0;
            g.done = S.done; g.redo = S.redo; g.cur = S.cur; g.first = S.first; g.method = S.method;
            g.lambda_solve = S.lambda_solve; g.lam_schur = schur_lambda(&S);
        } else {
            iter_prefetch2();
            // the solve's first launch: the starting state passes through to the buffer the next launch reads
            if (blockIdx.x == 0 && threadIdx.x < 64) {
                const double* src = reinterpret_cast<const double*>(dy.st_in);
                double* dst = reinterpret_cast<double*>(dy.st_out);
                for (int e = threadIdx.x; e < (int)(sizeof(DevState) / sizeof(double)); e += 64) dst[e] = src[e];
                if (threadIdx.x == 0) it.hs->word = status_word(dy.seq, 0, 0);
            }
            const DevState* st = dy.st_in;
            g.done = st->done; g.redo = st->redo; g.cur = st->cur; g.first = st->first; g.method = st->method;
            g.lambda_solve = st->lambda_solve; g.lam_schur = schur_lambda(st);
        }
    } else {
        const DevState* st = a.st;
        g.done = st->done; g.redo = st->redo; g.cur = st->cur; g.first = st->first; g.method = st->method;
        g.lambda_solve = st->lambda_solve; g.lam_schur = schur_lambda(st);
    }
    // the four wavefronts' rows -> the workgroup's row (fixed order), the two symmetric blocks as their upper triangles
    auto iter_row_out = [&]() {
        if constexpr (ITER) {
            __syncthreads();
            if (threadIdx.x < 64) for (int pe = threadIdx.x; pe < PROW; pe += 64) {
                const int e = iter_row_src(D - 6, pe);
                dy.partial_out[(int64_t)blockIdx.x * PROW + pe] = ((it_rows[0][e] + it_rows[1][e]) + it_rows[2][e]) + it_rows[3][e];
            }
        }
    };
    // fused elimination (launch_gram1v_t decides): no separate elimination launch; a re-elimination group then runs here too
    const bool fuse = !GEN && a.fuse_elim != 0;
    // the records in HBM are what a re-elimination group reads: Gauss-Newton never has one, so a fused GN group skips the stores
    const bool keep_rec = GEN || !fuse || g.method == CCAL_METHOD_LM;
    if (g.done || (g.redo && !fuse)) return;            // finished, or a re-elimination group without fusion (no evaluation)
    G1V_STAMP(1);                                           // the state has arrived
    const int camf = (GEN && a.obs_cam) ? a.obs_cam[fa_] : a.cam;          // GEN, merged launch: the frame's camera
    double* fcw = smem + wave * WSL;
    double* fc = fcw + grp * FC_N0P;
    double* red = fcw + G * FC_N0P;
    const int cur = g.cur, first = g.first;
    const int es = first ? cur : (cur ^ 1);
    if constexpr (!GEN) {
        constexpr int REC_ = praw_jl_off(K) + 9, GS_ = (REC_ + 6 * K1 + 1) & ~1;
        static_assert(G * GS_ <= 64 * LS, "the frames' records fit the reduction buffer");
        if (g.redo) {
            // re-elimination group (LM: rejected step or missed speculation): the accepted set's stored records, new damping
            double* R = red + grp * GS_;
            double mcv = 0.0;
            int slot_r = 0;
            if (active) {
                const double* rec = a.praw[cur] + (int64_t)f * a.PRAW;
                slot_r = a.obs_slot[f];
                for (int e = gl; e < REC_; e += LPF) R[e] = rec[e];
                if (gl == 0) mcv = a.mc_f[f];
            }
            wsync();
            gram_fused_tail<K, LPF>(a, g.lam_schur, red, ITER ? it_rows[wave] : a.partial + (int64_t)(blockIdx.x * WPB + wave) * fused_red_size(K), grp, gl, lane_ok, active, slot_r, cur, mcv);
            iter_row_out();
            return;
        }
    }
    double th[th_len<MODEL>()];
    if constexpr (ITER) {
        if (from_lds) load_theta<MODEL, OF>(hsh.cand, a.rt, th);           // the candidate this launch has just formed
        else load_theta<MODEL, OF>(a.intr[es], a.rt, th);
    } else {
        load_theta<MODEL, OF>(a.intr[es] + ((GEN && a.obs_cam) ? camf * CCAL_PMAX : 0), a.rt, th);
    }
    const int64_t start = ITER ? start_p : a.obs_off[fa_];
    const int n = ITER ? n_p : (active ? (int)(a.obs_off[fa_ + 1] - start) : 0);
    if constexpr (!ITER) {
        const int64_t g0 = start + (gl < n ? gl : 0);
        pX = a.x[g0]; pY = a.y[g0]; pZ = a.z[g0]; pU = a.u[g0]; pV = a.v[g0];
    }
    {
        // candidate pose of this group's frame (back-substitution of the previous camera solve) + constants;
        // the 16 lanes of a group compute the same values, the 4 groups work on 4 frames at once
        int slot;                           // (identity table: no round trip in front of the pose and the elimination record)
        if constexpr (ITER) slot = slot_p; else { if (!GEN && a.slot_ident) slot = fa_; else slot = a.obs_slot[fa_]; }
        double pose[6];
        if constexpr (ITER) {
#pragma unroll
            for (int i = 0; i < 6; ++i) pose[i] = cur ? pose_p[1][i] : pose_p[0][i];
            // the accepted set's elimination record of the frame's slot: from the lanes' registers into LDS (the reduction
            // buffer is free until the corner loop has ended)
            constexpr int PFS = (PFLEN + 1) & ~1;
            static_assert(G * PFS <= 64 * LS, "the frames' elimination records fit the reduction buffer");
            if (lane_ok) {
#pragma unroll
                for (int q = 0; q < NPFQ; ++q) if (gl + LPF * q < PFLEN) red[grp * PFS + gl + LPF * q] = cur ? pf_p[1][q] : pf_p[0][q];
            }
            wsync();
        } else {
            // GEN: k_backsub has formed the candidate - or, FusedArgs::gen_backsub, it is formed here from the accepted pose
            const bool gbs = GEN && a.gen_backsub != 0 && !first;
#pragma unroll
            for (int i = 0; i < 6; ++i) pose[i] = a.poses[(GEN && !gbs) ? es : cur][(int64_t)slot * 6 + i];
            if constexpr (GEN) {
                if (gbs) {
                    const double mcg = gen_backsub_pose<LPF, G, 64 * LS>(a, slot, g.lambda_solve, pose, red, grp, gl, lane_ok);
                    if (active && a.g_owner[fa_]) {
#pragma unroll
                        for (int i = 0; i < 6; ++i) if (gl == i) a.poses[es][(int64_t)slot * 6 + i] = pose[i];
                        if (gl == 0) a.g_mc_slot[slot] = mcg;
                    }
                }
            }
        }
        double mc = 0.0;
        if (!GEN && !first) {
            const double* pf;
            if constexpr (ITER) pf = red + grp * ((PFLEN + 1) & ~1); else pf = a.pf[cur] + (int64_t)slot * a.PF;
            double dcr[K];                                  // the camera step
            if constexpr (ITER) {
#pragma unroll
                for (int j = 0; j < K; ++j) dcr[j] = hsh.x[j];    // (not the first launch: this launch's own solve)
            } else {
#pragma unroll
                for (int j = 0; j < K; ++j) dcr[j] = a.dc[j];
            }
            if (pf[0] != 0.0) {
                double dp[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    const double* yr = pf + 21 + i * K1;
                    double t = yr[K];
#pragma unroll
                    for (int j = 0; j < K; ++j) t += yr[j] * dcr[j];
                    dp[i] = -t;
                }
#pragma unroll
                for (int i = 5; i >= 0; --i) {
                    double t = dp[i];
#pragma unroll
                    for (int k = i + 1; k < 6; ++k) t -= pf[k * (k + 1) / 2 + i] * dp[k];
                    dp[i] = t * pf[i * (i + 1) / 2 + i];
                }
                const double lam = g.lambda_solve;
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    const double gp = pf[21 + 6 * K1 + i], dCi = pf[21 + 6 * K1 + 6 + i];
                    const double Dii = lam > 0.0 ? lam * clampd1(dCi, a.min_diag, a.max_diag) : 0.0;
                    mc += dp[i] * (Dii * dp[i] - gp);
                    pose[i] += dp[i];
                }
            }
            if (active) {
#pragma unroll
                for (int i = 0; i < 6; ++i) if (gl == i) a.poses[es][(int64_t)slot * 6 + i] = pose[i];
            }
        }
        if constexpr (ITER) {
            if (fold_first && active) {            // k_unpack1's part of this frame: the starting pose into the parameter sets
#pragma unroll
                for (int i = 0; i < 6; ++i) if (gl == i) { if (!a.it.poses_on_device) a.poses[0][(int64_t)slot * 6 + i] = pose[i]; a.poses[1][(int64_t)slot * 6 + i] = pose[i]; }
            }
        }
        if (!GEN && active && gl == 0) a.mc_f[f] = mc;
        if constexpr (GEN) {
            // composed pose T_c0 o T_0b and the 6 x 12 expansion matrix E (frame_setup_composed); E^T goes straight into
            // the frame's record, where k_schur finds it
            const bool other = camf > 0;
            double ex[6], fcr[12], ept[GEN_EPT];
#pragma unroll
            for (int i = 0; i < 6; ++i) ex[i] = other ? a.extr[es][camf * 6 + i] : 0.0;
            frame_setup_composed(pose, ex, fcr, ept);
            if (gl == 0 && lane_ok) {
#pragma unroll
                for (int i = 0; i < 12; ++i) fc[i] = fcr[i];
            }
            if (gl == 0 && active) {
                double ec[GEN_EC];
                gen_et_compact(ept, ec);
                double2* rec = reinterpret_cast<double2*>(a.praw[es] + a.rec_off[fa_] + gen_e_off(K));
#pragma unroll
                for (int i = 0; i < GEN_EC / 2; ++i) rec[i] = make_double2(ec[2 * i], ec[2 * i + 1]);
            }
        } else {
            double fcr[FC_N0];
            frame_setup<false>(pose, nullptr, fcr);
            if (gl == 0 && lane_ok) {
#pragma unroll
                for (int i = 0; i < FC_N0; ++i) fc[i] = fcr[i];
            }
        }
    }
    wsync();
    G1V_STAMP(2);                                           // prologue done: frame constants in LDS

    double acc[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) acc[e] = 0.0;
    // same trip count for the whole wave: the largest frame of the four
    int nmax = n;
#pragma unroll
    for (int off = ((LPF & (LPF - 1)) == 0 ? LPF : 1); off < 64; off <<= 1) nmax = max(nmax, __shfl_xor(nmax, off, 64));
    for (int base = 0; base < nmax; base += LPF) {
        const int c = base + gl;
        const bool valid = c < n;
        const double X = pX, Y = pY, Z = pZ, uo = pU, vo = pV;
        if (base + LPF < nmax) {
            const int cn = base + LPF + gl;
            const int64_t gn = start + (cn < n ? cn : 0);
            pX = a.x[gn]; pY = a.y[gn]; pZ = a.z[gn]; pU = a.u[gn]; pV = a.v[gn];
        }
        double ru, rv, J[2 * D];
        corner_block<MODEL, OF, false, true>(th, fc, X, Y, Z, uo, vo, ru, rv, J, J + D);       // rotation columns in the phi basis
        const double sw = valid ? huber_sqrt_weight(ru * ru + rv * rv, a.huber_delta) : 0.0;
        // sqrt(w)-scaled rows (only the structurally non-zero entries are ever touched)
        double su[NC], sv[NC];
#pragma unroll
        for (int i = 0; i < D; ++i) { su[i] = sw * J[i]; sv[i] = sw * J[D + i]; }
        su[D] = sw * ru; sv[D] = sw * rv;
        int e = 0;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
#pragma unroll
            for (int j = i; j < NC; ++j) {
                const bool bu = (i >= K || nz_u<OF>(i)) && (j >= K || nz_u<OF>(j));
                const bool bv = (i >= K || nz_v<OF>(i)) && (j >= K || nz_v<OF>(j));
                if (bu) acc[e] = __builtin_fma(su[i], su[j], acc[e]);
                if (bv) acc[e] = __builtin_fma(sv[i], sv[j], acc[e]);
                ++e;
            }
        }
    }

    G1V_STAMP(3);                                           // corner loop done
    // 16 partial Grams per frame -> one, through LDS, in two halves of the triangle
    double res[2][NQ];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        wsync();
#pragma unroll
        for (int t = 0; t < HALF; ++t) { const int e = h * HALF + t; if (e < NE) red[lane * LS + t] = acc[e < NE ? e : 0]; }
        wsync();
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int idx = lane + 64 * q;                      // (group, entry) pairs
            double sum = 0.0;
            if (idx < G * HALF) {
                const int g = idx / HALF, t = idx - g * HALF;
                const double* src = red + (g * LPF) * LS + t;
#pragma unroll
                for (int l = 0; l < LPF; ++l) sum += src[l * LS];
            }
            res[h][q] = sum;
        }
    }
    G1V_STAMP(4);                                           // lane sums reduced
    // scatter the upper triangle into the compact record  C (21) | [B|g] (6 x K1) | A (K1 x K1)
    const int fbase = (blockIdx.x * WPB + wave) * G;
    // fused elimination: what its tail needs from memory is requested now, behind the reductions
    int slot_t = 0;
    double mc_t = 0.0;
    if constexpr (!GEN) {
        if (fuse && active) { slot_t = a.obs_slot[f]; if (gl == 0) mc_t = a.mc_f[f]; }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int idx = lane + 64 * q;
            if (idx >= G * HALF) continue;
            const int g = idx / HALF, t = idx - g * HALF, e = h * HALF + t;
            const int ff = fbase + g;
            if (e >= NE || ff >= a.n_obs) continue;
            const uint32_t m = g_recmap<K, GEN>.d[e];
            const double v = res[h][q];
            double* rec = a.praw[es] + (GEN ? a.rec_off[a.list[ff]] : (int64_t)ff * a.PRAW);
            if (keep_rec) {
                rec[m & 0xffff] = v;
                if ((m >> 16) != 0xffff) rec[m >> 16] = v;
                if (!GEN && e == NE - 1) a.cost_f[ff] = v;               // the last entry is r x r
            }
            if constexpr (!GEN) {
                if (fuse) {                                          // fused elimination: the same record in LDS (red is free: every sum is in registers)
                    constexpr int GS_ = (praw_jl_off(K) + 9 + 6 * K1 + 1) & ~1;
                    red[g * GS_ + (m & 0xffff)] = v;
                    if ((m >> 16) != 0xffff) red[g * GS_ + (m >> 16)] = v;
                }
            }
        }
    }
    // the frame's left Jacobian (phi -> rvec map of the elimination)
    if (!GEN && active && keep_rec) for (int e = gl; e < 9; e += LPF) a.praw[es][(int64_t)f * a.PRAW + praw_jl_off(K) + e] = fc[FC_A + e];
    if constexpr (!GEN) {
        if (fuse) {
            constexpr int GS_ = (praw_jl_off(K) + 9 + 6 * K1 + 1) & ~1;
            if (lane_ok) for (int e = gl; e < 9; e += LPF) red[grp * GS_ + praw_jl_off(K) + e] = fc[FC_A + e];
            wsync();
            G1V_STAMP(5);                                   // record assembled (LDS and / or HBM)
            gram_fused_tail<K, LPF>(a, g.lam_schur, red, ITER ? it_rows[wave] : a.partial + (int64_t)(blockIdx.x * WPB + wave) * fused_red_size(K), grp, gl, lane_ok, active, slot_t, es, mc_t);
            iter_row_out();
        }
    }
#ifdef CCAL_STAMPS
    if (!GEN && lane == 0) { ts[6] = wall_clock64(); const int wg = blockIdx.x * WPB + wave; for (int i = 0; i < 10; ++i) a.fcbuf[16 * wg + i] = (double)ts[i]; }
#endif
#undef G1V_STAMP
}
template <int MODEL, bool OF, int LPF, bool GEN, bool ITER = false>
__global__ __launch_bounds__(64 * (ITER ? 4 : CCAL_GRAMV_WPB), 1) void k_gram1v(const FusedArgs) {
    // The argument block is read where it lies - the kernarg segment, offset 0 - through a pointer: handing the by-value parameter
    // to the (inlined) body by reference made the compiler copy all 1 088 bytes of it into scratch, because the body indexes its
    // pointer arrays (a.intr[set], a.poses[set], ...) at run time; a pointer into constant memory keeps those scalar loads at a
    // computed offset, which is also exactly what the batched kernel below does with its table.
    const FusedArgs& a = *(const FusedArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    IterDyn dy = {};
    if constexpr (ITER) {
        dy.seq = a.it.seq; dy.skip_head = a.it.skip_head; dy.fold = a.it.fold;
        dy.st_in = a.it.st_in; dy.st_out = a.it.st_out; dy.partial_in = a.it.partial_in; dy.partial_out = a.partial;
    }
    gram1v_body<MODEL, OF, LPF, GEN, ITER>(a, dy);
}
// ccal_solve_batch: ONE launch per optimizer step for a whole batch of session-sized problems (same model, focal mode and lane
// mapping): blockIdx.y = the problem, `tab` = the problems' argument blocks in device memory, written once per batch; what a
// single-problem launch finds in IterArgs per step follows from the launch number s here - the two state buffers and the two
// halves of the partial-sum buffer alternate by s (tab[.].it.st_in / tab[.].partial: their bases), the first launch has nothing to
// decide and (it.fold) unpacks the starting point.  n problems x 4 launches per solve from n host threads were serialised by the
// runtime's launch path (eight 625-frame sessions: 0.48 ms per batch for ~0.1 ms of device work); this is 4-5 launches per BATCH.
template <int MODEL, bool OF, int LPF>
__global__ __launch_bounds__(256, 1) void k_gram1v_batch(const FusedArgs* __restrict__ tab, const int s) {
    const FusedArgs& a = tab[blockIdx.y];
    if ((int)blockIdx.x >= a.n_part) return;                   // (problems of a batch differ in size: the grid is the largest one's)
    constexpr int RB1 = fused_red_size(block_dim(MODEL, OF, false) - 6);
    IterDyn dy;
    dy.seq = s; dy.skip_head = s == 1 ? 1 : 0; dy.fold = (s == 1 && a.it.fold != 0) ? 1 : 0;
    DevState* const sb = const_cast<DevState*>(a.it.st_in);
    dy.st_in = sb + (s & 1); dy.st_out = sb + ((s + 1) & 1);
    const size_t half = (size_t)a.n_part * RB1;
    dy.partial_in = a.partial + (size_t)((s - 1) & 1) * half; dy.partial_out = a.partial + (size_t)(s & 1) * half;
    gram1v_body<MODEL, OF, LPF, false, true>(a, dy);
}

template <int MODEL, bool OF, int LPF, bool GEN>
static hipError_t launch_gram1v_l(const FusedArgs& a, hipStream_t s) {
    constexpr int G = 64 / LPF;
    const size_t lds = sizeof(double) * gram1_wave_lds<MODEL, OF>(LPF) * CCAL_GRAMV_WPB;
    void (*kern)(const FusedArgs) = k_gram1v<MODEL, OF, LPF, GEN>;
    static DynLdsGuard lds_guard;
    if (hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(kern), lds, lds_guard); e != hipSuccess) return e;
    const int fpb = G * CCAL_GRAMV_WPB;
    if (a.n_obs <= 0) return hipSuccess;
    hipLaunchKernelGGL(kern, dim3((a.n_obs + fpb - 1) / fpb), dim3(64 * CCAL_GRAMV_WPB), lds, s, a);
    return hipGetLastError();
}
// Lanes per frame: the cost model of ccal_gram_plan.hpp with k_gram1v's constants (one wavefront per SIMD).
// The second library's CCAL_GRAMV_LPF overrides.
static int gram_lanes_per_frame(int n_obs, int avg_corners, int64_t max_waves = kNoWaveCap, int share = 1) {
    static const int lpf_env = dev_env_int("CCAL_GRAMV_LPF", 0);
    return lanes_per_frame(n_obs, avg_corners, gram1_lane_cost(false), lpf_env, max_waves, share);
}
template <int MODEL, bool OF, bool GEN>
static hipError_t launch_gram1v_t(FusedArgs& a, hipStream_t s) {
    const int lpf = gram_lanes_per_frame(a.n_obs, a.avg_corners, fused_wave_cap(a, GEN), a.share);
    set_fuse_plan(a, lpf, GEN);
    return dispatch_lanes(lpf, hipErrorInvalidValue, [&](auto l) { return launch_gram1v_l<MODEL, OF, decltype(l)::value, GEN>(a, s); });
}
template <bool GEN>
static hipError_t launch_gram1v_m(int model, bool one_focal, FusedArgs& a, hipStream_t s) {
    return dispatch_model_focal(model, one_focal, hipErrorInvalidValue, [&](auto m, auto of) {
        constexpr int MODEL = decltype(m)::value;
        if constexpr (MODEL == kOCV5) return hipErrorNotSupported;          // (OPENCV5: k_gram2 for every size, use_gram2)
        else return launch_gram1v_t<MODEL, decltype(of)::value, GEN>(a, s);
    });
}
// ---- single-launch groups (k_gram1v<.., ITER>) ----
constexpr int kIterWpb = 4;
constexpr size_t kLdsPerCu = 160 * 1024;
template <int MODEL, bool OF>
static constexpr size_t iter_lds_bytes(int lpf) { return sizeof(double) * gram1_wave_lds<MODEL, OF>(lpf) * kIterWpb; }
template <int MODEL, bool OF, int LPF>
static hipError_t launch_gram_iter_l(FusedArgs& a, hipStream_t s) {
    constexpr int G = 64 / LPF;
    const size_t lds = iter_lds_bytes<MODEL, OF>(LPF);
    void (*kern)(const FusedArgs) = k_gram1v<MODEL, OF, LPF, false, true>;
    static DynLdsGuard lds_guard;
    if (hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(kern), lds, lds_guard); e != hipSuccess) return e;
    const int fpb = G * kIterWpb;
    a.fuse_elim = 1; a.elim_fused = 1;
    a.n_part = (a.n_obs + fpb - 1) / fpb;
    hipLaunchKernelGGL(kern, dim3(a.n_part), dim3(64 * kIterWpb), lds, s, a);
    return hipGetLastError();
}
// static LDS of the ITER form beside the dynamic part: HeadShared + the reduction's 4 x 64 + the four rows
template <int MODEL, bool OF>
static constexpr size_t iter_static_lds() { return sizeof(HeadShared) + 4 * 2 * 64 * 8 + 4 * 8 * (size_t)fused_red_size(block_dim(MODEL, OF, false) - 6) + 256; }
// rows (= workgroups) of a single-launch group, 0 if the form does not apply; launch: the group is launched as well (*err)
template <int MODEL, bool OF>
static int iter_rows_t(int n_obs, int avg_corners, int share, bool launch, FusedArgs* a, hipStream_t s, hipError_t* err) {
    // OPENCV5: only the batched form exists (k_gram1v_batch) - the row count without the single-problem launcher
    constexpr bool LAUNCHER = MODEL != kOCV5;
    // CCAL_ITER_ROWS: most rows (= workgroups, each of which reads every row of the launch before) for which a group is one
    // launch; 0 = never.  One wavefront per SIMD, every workgroup resident at once: <= 256 workgroups.
    static const int max_rows = std::min(dev_env_int("CCAL_ITER_ROWS", 256), 256);
    if (n_obs <= 0 || max_rows <= 0 || (launch && !LAUNCHER)) return 0;
    const int lpf = gram_lanes_per_frame(n_obs, avg_corners, kNoWaveCap, share);
    const int g = 64 / lpf, rows = (n_obs + g * kIterWpb - 1) / (g * kIterWpb);
    if (rows > max_rows || iter_lds_bytes<MODEL, OF>(lpf) + iter_static_lds<MODEL, OF>() > kLdsPerCu) return 0;
    if constexpr (LAUNCHER) {
        if (launch) *err = dispatch_lanes(lpf, hipErrorInvalidValue, [&](auto l) { return launch_gram_iter_l<MODEL, OF, decltype(l)::value>(*a, s); });
    }
    return rows;
}
static int iter_rows_m(int model, bool one_focal, int n_obs, int avg_corners, int share, bool launch, FusedArgs* a, hipStream_t s, hipError_t* err) {
    return dispatch_model_focal(model, one_focal, 0, [&](auto m, auto of) {
        return iter_rows_t<decltype(m)::value, decltype(of)::value>(n_obs, avg_corners, share, launch, a, s, err);
    });
}
// ---- the batched form (k_gram1v_batch) ----
template <int MODEL, bool OF, int LPF>
static hipError_t launch_iter_batch_l(const FusedArgs* tab, int n, int max_rows, int s_no, hipStream_t s) {
    const size_t lds = iter_lds_bytes<MODEL, OF>(LPF);
    if (lds + iter_static_lds<MODEL, OF>() > kLdsPerCu) return hipErrorInvalidValue;
    void (*kern)(const FusedArgs*, int) = k_gram1v_batch<MODEL, OF, LPF>;
    static DynLdsGuard lds_guard;
    if (hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(kern), lds, lds_guard); e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(max_rows, n), dim3(64 * kIterWpb), lds, s, tab, s_no);
    return hipGetLastError();
}
// one launch for n problems of one model / focal mode / lane mapping; tab: device memory, n FusedArgs (bases, see the kernel)
hipError_t launch_gram_iter_batch(int model, bool one_focal, int lpf, const FusedArgs* tab, int n, int max_rows, int s_no, hipStream_t s) {
    return dispatch_model_focal(model, one_focal, hipErrorNotSupported, [&](auto m, auto of) {
        return dispatch_lanes(lpf, hipErrorInvalidValue, [&](auto l) {
            return launch_iter_batch_l<decltype(m)::value, decltype(of)::value, decltype(l)::value>(tab, n, max_rows, s_no, s);
        });
    });
}
// the lane mapping a single-launch group of this problem takes (what launch_gram_iter dispatches on)
int fused_iter_lpf(int n_obs, int avg_corners, int share) { return gram_lanes_per_frame(n_obs, avg_corners, kNoWaveCap, share); }

// CCAL_GRAM2_ITER=0 (second library) / -DCCAL_NO_GRAM2_ITER (A/B builds): k_gram1v's single-launch form at every size
static bool use_gram2_iter(bool batch, int share) {
#ifdef CCAL_NO_GRAM2_ITER
    return false;
#else
    static const bool on = dev_env_int("CCAL_GRAM2_ITER", 1) != 0 && dev_env_int("CCAL_ITER_ROWS", 256) > 0;      // (CCAL_ITER_ROWS=0: no single-launch groups at all)
    return on && !batch && share <= 1;
#endif
}
int fused_iter_rows(int model, bool one_focal, int n_obs, int avg_corners, int K, int share, bool batch) {
    if (K != block_dim(model, one_focal, false) - 6) return 0;      // (the kernel's compile-time column count is the problem's)
    // OPENCV5 alone: k_gram2 (fewer AGPR copies) + reduce + head stays ahead - 625 frames GN 0.132 ms against 0.139 in the single-launch
    // form (112-double rows: two chunks per lane to sum, 4.9 us) - so only members of a lockstep batch take it (one launch per step
    // for the whole batch beats n x three).
    if (model == kOCV5 && !batch) return 0;
    // UCM / EUCM from 2 000 frames, a problem that has the GPU to itself: the single-launch form of the two-wavefronts-per-SIMD kernel
    // (k_gram2i, ccal_kernels_gram2.hip) - 10 000 frames: ~30 us per group against 36 with k_gram1v's 1 000 one-per-SIMD wavefronts
    if (use_gram2_iter(batch, share)) { const int r = gram2_iter_rows(model, one_focal, n_obs, avg_corners, K); if (r > 0) return r; }
    return iter_rows_m(model, one_focal, n_obs, avg_corners, share, false, nullptr, nullptr, nullptr);
}
hipError_t launch_gram_iter(int model, bool one_focal, FusedArgs& a, hipStream_t s) {
    if (use_gram2_iter(false, a.share) && gram2_iter_rows(model, one_focal, a.n_obs, a.avg_corners, a.K) > 0) return launch_gram2_iter(model, one_focal, a, s);
    hipError_t err = hipErrorInvalidValue;
    const int rows = iter_rows_m(model, one_focal, a.n_obs, a.avg_corners, a.share, true, &a, s, &err);
    return rows > 0 ? err : hipErrorInvalidValue;
}

// single-camera loop; a.fuse_elim in: fusion allowed, out: fusion done (then a.n_part = rows of partial sums, a.elim_fused = 1)
// Which register Gram kernel.  k_gram2 (the block's rows on neighbouring lanes, ccal_kernels_gram2.hip) where it measured faster
// (10 000 / 2 500 frames, us per build, k_gram2 vs k_gram1v): OPENCV5 47.1 / 25.6 vs 51.2 / 27.3, EUCM 35.8 / 21.1 vs 36.9 / 22.2
// (from 2 000 frames: two wavefronts per SIMD, no LDS accumulators; 625 frames 15.9 vs 14.2 with k_gram1v); KB4 since round 5
// (neighbouring-lane form): 46.7 / 24.4 vs 49.7 / 25.8, one focal 45.9 vs 47.2.  CCAL_GRAM2=0|1 forces (second library) for
// UCM / EUCM / KB4.  OPENCV5 takes k_gram2 whatever the switch says: k_gram1v has no single-problem instantiation for it.
static bool use_gram2(int model, int n_obs) {
    static const int force = [] { const char* e = dev_env("CCAL_GRAM2"); return e ? (e[0] == '1' ? 1 : 0) : -1; }();
    if (model == kOCV5) return true;
    if (force >= 0) return force == 1;
    return n_obs >= 2000;
}
static int gram2_lpf_force() { static const int v = dev_env_int("CCAL_GRAM2_LPF", 0); return v; }
hipError_t launch_gram1v(int model, bool one_focal, FusedArgs& a, hipStream_t s) {
    if (use_gram2(model, a.n_obs)) { a.lpf_force = gram2_lpf_force(); return launch_gram2(model, one_focal, a, s); }
    return launch_gram1v_m<false>(model, one_focal, a, s);
}
// one camera's blocks of a multi-camera problem: a.list / a.rec_off / a.n_obs = that camera's observation frames
hipError_t launch_gram1v_general(int model, bool one_focal, const FusedArgs& a0, hipStream_t s) {
    FusedArgs a = a0; a.fuse_elim = 0;
    if (use_gram2(model, a0.n_obs)) { a.lpf_force = gram2_lpf_force(); return launch_gram2_general(model, one_focal, a, s); }
    return launch_gram1v_m<true>(model, one_focal, a, s);
}
// ---------------------------------------------------------------------------------------------
// k_reduce1: red[e] = sum over workgroups of partial[w][e], fixed order (no atomics: bitwise reproducible)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_reduce1(const double* partial, int n_part, int rb, double* red, const DevState* st) {
    if (st->done) return;
    __shared__ double sh[4][64];
    const int e = blockIdx.x * 64 + (threadIdx.x & 63);
    const double t = reduce_partial_rows(partial, n_part, rb, e, sh);
    if (threadIdx.x < 64 && e < rb) red[e] = t;
}
// Many rows (> kHeadReduceRows, where k_head never reduces itself): one workgroup per entry, 256 threads over the rows,
// shuffle tree + four wavefront sums - the parallel form (10 000 frames = 313 rows: 4.4 us instead of 7.8)
__global__ __launch_bounds__(256) void k_reduce1_wide(const double* partial, int n_part, int rb, double* red, const DevState* st) {
    if (st->done) return;
    __shared__ double sh[4];
    const double* src = partial + blockIdx.x;
    double v0 = 0.0, v1 = 0.0;
    int r = threadIdx.x;
    for (; r + 256 < n_part; r += 512) { v0 += src[(int64_t)r * rb]; v1 += src[(int64_t)(r + 256) * rb]; }
    if (r < n_part) v0 += src[(int64_t)r * rb];
    double v = v0 + v1;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) red[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
hipError_t launch_reduce1(const FusedArgs& a, hipStream_t s) {
    const int rb = fused_red_size(a.K);
    // up to kHeadReduceRows rows the order must be k_head's own (reduce_partial_rows): sharded and single-GPU solves of the
    // same frames then agree bit for bit; beyond, both go through the wide form
    if (a.n_part <= kHeadReduceRows) hipLaunchKernelGGL(k_reduce1, dim3((rb + 63) / 64), dim3(256), 0, s, a.partial, a.n_part, rb, a.red, a.st);
    else hipLaunchKernelGGL(k_reduce1_wide, dim3(rb), dim3(256), 0, s, a.partial, a.n_part, rb, a.red, a.st);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// k_head: one wavefront.  Decision (optimizer_decide, ccal_fused.hpp) on the all-reduced sums, then - when the sums at
// hand are the system to solve - the K x K camera solve and the candidate intrinsics.
// red = [A_dir (K1*K1) | Y^T Y (K1*K1) | mc_pose | failed pose blocks]
// The optimizer state is staged in LDS once (the global copy is touched twice per launch).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_head(const HeadArgs a) {
    __shared__ HeadShared hs;
    if (a.partial) {
        // single-GPU loop: the partial sums of the elimination kernel are added up here in k_reduce1's order (a launch and a
        // kernel boundary less per group); then wavefront 0 decides alone
        if (a.st->done) { if (threadIdx.x == 0) publish_host_status(a.hs, a.st, a.seq, a.publish_all != 0); return; }
        __shared__ double shr[4][64];
        const int rb = fused_red_size(a.K);
        for (int e0 = 0; e0 < rb; e0 += 64) {
            const int e = e0 + (threadIdx.x & 63);
            const double t = reduce_partial_rows(a.partial, a.n_part, rb, e, shr);
            if (threadIdx.x < 64 && e < rb) hs.red[e] = t;
        }
        __syncthreads();
    } else if (a.peers.n > 0) {
        // in-process transport: this step's sums of every rank, added here in rank order (no launch, no buffer in between)
        if (a.st->done) { if (threadIdx.x == 0) publish_host_status(a.hs, a.st, a.seq, a.publish_all != 0); return; }
        const int rb = fused_red_size(a.K);
        for (int e = threadIdx.x; e < rb; e += 256) hs.red[e] = peer_sum(a.peers, e);
        __syncthreads();
    }
    HeadIO io;
    io.st_in = a.st; io.st_out = a.st; io.hs = a.hs; io.red_g = (a.partial || a.peers.n > 0) ? nullptr : a.red; io.cols = a.cols;
    io.intr[0] = a.intr[0]; io.intr[1] = a.intr[1]; io.dc = a.dc; io.K = a.K; io.seq = a.seq;
    io.min_diag = a.min_diag; io.max_diag = a.max_diag; io.publish_all = a.publish_all;
    if (threadIdx.x < 64) head_wave(io, hs, (int)threadIdx.x, true, head_prefetch(io, (int)threadIdx.x));
    __syncthreads();
    head_finish(io, hs, a.result_host, a.poses[0], a.poses[1], a.np6, true);
}
// ccal_build_normal_dev on a single camera: evaluate set 0 as a first evaluation (no pose update) with this damping
__global__ void k_state_eval(DevState* st, double lambda) {
    st->done = 0; st->cur = 0; st->first = 1; st->redo = 0; st->iter = 0;
    st->lambda = lambda; st->lambda_spec = lambda; st->lambda_solve = 0.0;
    st->method = lambda > 0.0 ? CCAL_METHOD_LM : CCAL_METHOD_GN;
}
hipError_t launch_state_eval(DevState* st, double lambda, hipStream_t s) {
    hipLaunchKernelGGL(k_state_eval, dim3(1), dim3(1), 0, s, st, lambda);
    return hipGetLastError();
}
hipError_t launch_head(const HeadArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_head, dim3(1), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace ccal

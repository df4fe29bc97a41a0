// Mode N (normal equations + exact per-frame Schur complement) and solver-loop workspaces.
//
// Pipeline of one linear solve (all on the context stream, everything stays in HBM):
//   k_gram    per observation frame: G_o = [J|r]^T W [J|r] with v_mfma_f64_16x16x4_f64   (heavy)
//   k_schur   per frame slot: assemble C = H_pp, B = [H_pc | g_p], eliminate the pose block,
//             accumulate the reduced system in per-wave LDS accumulators, keep L and Y = L^-1 B
//   k_reduce  deterministic sum of the per-wave partials -> red[RB]      (the all-reduce buffer)
//   k_solve   one workgroup: damping, fixed mask, Cholesky K x K, dc, clamp to bounds
//   k_backsub per slot: dp = -L^-T (y_r + Y dc), candidate poses, model-decrease partials
#pragma once
#include "ccal_internal.hpp"

#ifndef CCAL_GRAM_TILE
#define CCAL_GRAM_TILE 32
#endif
#ifndef CCAL_GRAM_MINW
#define CCAL_GRAM_MINW 1          // launch_bounds: minimum wavefronts per SIMD the Gram kernels are compiled for
#endif

namespace ccal {

// corners whose weighted rows are staged in LDS at a time by the Gram kernels (32 or 64)
constexpr int GRAM_TILE_CORNERS = CCAL_GRAM_TILE;

// layout of the reduced buffer red[RB]:  A[(K+1)*(K+1)] | hdiag[K] | gc[K] | cost | mc_pose | failed pose blocks
//   A = [[S, b],[b^T, *]] undamped in the camera block (pose damping already inside the Schur terms)
inline int red_size(int K) { return (K + 1) * (K + 1) + 2 * K + 3; }
// per-slot record pf[PF]: L (21, row-major lower, diagonal stored inverted) | Y[6][K+1] | g_p[6] | dC[6]
inline int pf_size(int K) { return (21 + 6 * (K + 1) + 12 + 1) & ~1; }

struct ColInfo {          // one column of the reduced camera system
    double lo, hi;
    int32_t has_bound, fixed;
    int32_t is_extr;      // 0: intrinsic (index into intr, full layout), 1: extrinsic (index into extr)
    int32_t dst, dst2;    // element index in the destination array; dst2 >= 0 mirrors the value (fy = f)
};

struct DevState {                 // lives in device memory; updated by the decision kernels only (sizeof % 8 == 0)
    double lambda;                // damping of the system to solve next (0 for GN)
    double lambda_spec;           // LM: damping of the speculative elimination at the candidate
    double lambda_solve;          // damping that produced the current dc (model decrease of the pose blocks)
    double radius, dec;
    double cur_cost, last_cost, initial_cost;
    double mc_cam;                // model decrease of the camera block for the current dc
    double min_error, min_abs, min_rel;
    int32_t cur;                  // parameter set (0/1) holding the accepted point
    int32_t first;                // 1 until the starting point has been evaluated
    int32_t redo;                 // 1: the next group re-eliminates the accepted set with `lambda` (no evaluation, no decision)
    int32_t done;                 // 0 = running, else ccal_status + 1
    int32_t iter, max_iter, method;
    int32_t lm_accepted, lm_rejected;
    int32_t sys_failed;           // a pose block of the system that produced the candidate was not positive definite (any rank)
    int32_t cam_failed;           // the camera system that produced the candidate was not positive definite
    int32_t done_seq;             // sequence number of the step that set `done` (0 while running)
    int32_t spec_hits, spec_misses;   // LM: accepted steps whose speculative elimination was / was not the next system
    int32_t error_metric;         // ccal_solver_opts::error_metric: what the stop rules compare (0: cost, 1: its square root)
    int32_t pad_;
};
static_assert(sizeof(DevState) % 8 == 0, "DevState is staged as doubles");

struct HostStatus {               // pinned, host-coherent; written at the end of a decision kernel
    // what the polling host needs after EVERY group, in one 8-byte store (no fence, no second word to order against):
    // bits 0-23 sequence number of the group, 24-31 `done` (0 = running, else ccal_status + 1), 32-55 the sequence number
    // of the step that set `done` - the host acts on `done` only once it has waited for that step
    volatile uint64_t word;
    // the rest is published (behind a system-scope fence, before `word`) only by the group that finishes the solve
    volatile int32_t iter, cur, lm_accepted, lm_rejected;
    volatile int32_t spec_hits, spec_misses;
    volatile double cur_cost, initial_cost, radius;
};
struct NormalWs {
    int K = 0, RB = 0, PF = 0, n_pw = 0;
    // the candidate poses are formed in the GEN Gram kernels' prologue (FusedArgs::gen_backsub) instead of by k_backsub: set by the
    // device-resident general loop for its launches (CCAL_GEN_BACKSUB=0: the separate launch); d_obs_owner[o] = 1 for the first
    // observation frame of its slot (the one that writes the candidate pose and the model decrease)
    bool gen_backsub = false; double lm_min_diag = 1e-6, lm_max_diag = 1e32;
    int8_t* d_obs_owner = nullptr;
    bool all_slots_observed = false;           // no slot without an observation frame: the two pose sets need not start equal
    bool general_ready = false;                // the general loop's buffers exist (normal_ws_ensure_general); the single-camera loop never asks
    int schur_wpb = 4;                         // wavefronts per workgroup of k_schur: 1 for reduced systems of 64 .. 127 columns
    bool schurq = false;                       // two cameras with equal blocks: elimination with four lanes per slot (k_schurq) instead of k_schur<true>
    int schurq_slots = 16;                     // k_schurq: frame slots per wavefront (16 = four lanes each, 8 = eight lanes each)
    int n_rows = 0;                            // rows of partial sums the elimination kernel in use writes = what k_reduce adds up
    // three blocks (NormalBaseLayout, GeneralLayout below): d_base = dc | cols, what every loop needs; d_block and the pinned, host-coherent
    // h_block = the general loop's buffers, made when a general-loop entry first asks.  Every pointer below is a slice of one of them.
    char* d_base = nullptr; char* d_block = nullptr; char* h_block = nullptr;
    double* G[2] = { nullptr, nullptr };       // per-observation-frame Gram blocks (current / candidate)
    double* cost_o[2] = { nullptr, nullptr };  // per-observation-frame cost
    int64_t* d_goff = nullptr;                 // [n_obs] offset of G_o
    int32_t* d_slot_off = nullptr;             // [n_slots+1] CSR slot -> observation frames
    int32_t* d_slot_obs = nullptr;
    int32_t* d_all_obs = nullptr;              // merged Gram launch: every camera's observation frames, camera-major
    bool merged_gram = false;                  // all cameras share model and focal mode: their blocks in ONE launch of the register Gram kernel
    // ragged frames (round 6): a Gram launch's list of observation frames sorted by corner count + the bins of the launch (gram2_bin_plan);
    // [0]: the merged launch, [1 + c]: camera c's own launch.  n_bins == 0: the plain launch over the list in table order
    GramBins gen_bins[1 + CCAL_MAX_CAMS];
    int32_t* d_gen_sorted[1 + CCAL_MAX_CAMS] = {};
    int64_t* d_slot_rec = nullptr;             // k_schurq: [n_slots][2] record offset of camera 0 / 1 in that slot, -1 = none
    int64_t* d_slot_desc = nullptr;            // [n_obs] in slot order: goff * 8 + camera
    int32_t* d_obs_cam = nullptr;
    int32_t* d_caminfo = nullptr;              // [n_cams][4]: Peff, col_theta, col_extr, NCP
    double* partial = nullptr;                 // [RB][n_pw]
    double* red = nullptr;                     // [2][RB + 8]: the reduced sums; the in-process transport alternates between the two
    double* red_out = nullptr;                 // where this group's k_reduce writes (NULL: red)
    PeerView peers = {};                       // this group's k_solve: every rank's sums (in-process transport), n == 0: red
    double* pf = nullptr;                      // [n_slots][PF]
    double* dc = nullptr;                      // [K]
    double* mc_slot = nullptr;                 // [n_slots]
    double* scal = nullptr;                    // [8]: 2 = model decrease of the camera block (host-driven form)
    int32_t* flags = nullptr;                  // [4]: 1 = camera Cholesky failed (host-driven ccal_build_normal form only)
    ColInfo* cols = nullptr;                   // [K]
    double* h_pinned = nullptr;                // pinned staging (RB + 16 doubles): ccal_build_normal's host form reads the sums here
    int cur = 0;                               // which G buffer holds the current point
    bool red_fused = false;                    // the last ccal_build_normal_dev left its sums in fws->red (single camera)
    bool gstate_is_eval = false;               // d_gstate already says "first evaluation of set 0" (ccal_build_normal)
    bool register_gram = false;                // general loop: every camera's blocks come from k_gram1v / k_gram2 (GEN record format, caminfo NCP = 0)
    int64_t g_len = 0;
    DevState* d_gstate = nullptr;              // general loop: optimizer state on the device,
    HostStatus* h_gstatus = nullptr;           //   its published copy (pinned, host-coherent)
    DevState* h_gstate = nullptr;              //   and the pinned staging of its initial value
    hipStream_t side = nullptr;                // result download past the early-exit group enqueued ahead
    bool tail_pending = false;
    struct FusedWs* fws = nullptr;             // single-camera fused path (ccal_fused.hpp)
};

struct FusedWs {
    int PRAW = 0, RB1 = 0, n_pw = 0;
    char* d_block = nullptr;                   // the ONE device allocation the buffers below are slices of (fcbuf apart)
    char* h_block = nullptr;                   // the ONE pinned, host-coherent allocation: h_status | h_result | h_stage
    double* pf[2] = { nullptr, nullptr };
    double* praw[2] = { nullptr, nullptr };
    double* partial = nullptr;
    double* red = nullptr;                     // [2][RB1 + 7 rounded]: the in-process transport alternates between the two (red_stride apart)
    size_t red_stride = 0;
    double* fcbuf = nullptr;                   // -DCCAL_STAMPS builds only: in-kernel timestamps (NULL in the product build)
    double* mc_f = nullptr;                    // [n_obs] model decrease of each pose block
    double* cost_f = nullptr;                  // [n_obs] cost of each frame
    DevState* d_state = nullptr;
    bool state_is_eval = false; double state_eval_lambda = 0.0;     // d_state already says "first evaluation of set 0" with this damping
    bool fuse_elim = true;                     // the Gram kernels eliminate their frames' pose blocks in their tail (second library, CCAL_FUSE_ELIM=0: separate launch)
    HostStatus* h_status = nullptr;            // pinned, host-coherent
    double* h_stage = nullptr;                 // pinned staging of the caller's poses (read by k_unpack1 in place when small)
    double* d_stage = nullptr;                 // their device image (large problems: one copy per solve, k_unpack1 distributes it)
    double* h_result = nullptr;                // pinned, host-coherent: [intr | poses] written by the k_head that finishes a session-sized solve
                                               // (up to kSpreadBytes of poses: by every workgroup of a finishing single-launch group, head_finish SPREAD)
    int32_t* done_cnt = nullptr;               // SPREAD: the workgroups that have written their slice (zero between solves)
    hipStream_t side = nullptr;                // result download: does not queue behind the early-exit groups
    bool tail_pending = false;                 // early-exit groups of the previous solve may still be in flight
    int all_slots_observed = -1;               // every frame slot has an observation frame (-1: not looked yet): the first single-launch group may unpack for itself
};

// ---- the workspaces' blocks, each described ONCE: the layout's constructor declares the slices in order - cleared ones first, slices
// of doubles marked for the test hook - and size, pointers, the one clear and the poison ranges follow (ccal_plan.hpp,
// ctx_block_alloc).  A new slice: declare it here, bind it in the ensure function, done.  Pure arithmetic: tests/cpp/test_ws_layouts.cpp
struct NormalBaseLayout {
    CallPlan plan; Slice<double> dc; Slice<ColInfo> cols;
    NormalBaseLayout() { dc = plan.add<double, kDoubles>(CCAL_KMAX); cols = plan.add<ColInfo>(CCAL_KMAX); }
};

struct GeneralLayout {
    CallPlan dev, host;
    Slice<double> G[2], cost_o[2], partial, mc_slot, scal; Slice<int32_t> flags;      // cleared: what the kernels never write must stay zero
    Slice<double> red, pf; Slice<DevState> gstate;
    // the index tables: one host image, one copy ([goff.off, dev.total))
    Slice<int64_t> goff; Slice<int32_t> slot_off, slot_obs, obs_cam, caminfo; Slice<int64_t> slot_desc; Slice<int8_t> obs_owner;
    Slice<int32_t> all_obs; Slice<int64_t> slot_rec; Slice<int32_t> sorted[1 + CCAL_MAX_CAMS];
    Slice<HostStatus> h_gstatus; Slice<DevState> h_gstate; Slice<double> h_pinned;
    // part_rows: the most rows of `partial` an elimination kernel writes; merged / schurq: d_all_obs / d_slot_rec exist; n_sorted[i]: 0 = none
    GeneralLayout(int n_cams, size_t n_obs, size_t n_slots, size_t RB, size_t PF, size_t g_len, size_t part_rows, bool merged, bool schurq,
                  const size_t* n_sorted) {
        constexpr unsigned kCD = kCleared | kDoubles;
        const size_t no = std::max<size_t>(n_obs, 1), ns = std::max<size_t>(n_slots, 1);
        for (auto& g : G) g = dev.add<double, kCD>(std::max<size_t>(g_len, 1));
        for (auto& c : cost_o) c = dev.add<double, kCD>(no);
        partial = dev.add<double, kCD>(RB * part_rows); mc_slot = dev.add<double, kCD>(ns);
        scal = dev.add<double, kCD>(8); flags = dev.add<int32_t, kCleared>(4);
        red = dev.add<double, kDoubles>(2 * (RB + 8));        // two buffers RB + 8 apart: the in-process transport alternates
        pf = dev.add<double, kDoubles>(ns * PF); gstate = dev.add<DevState>(1);
        goff = dev.add<int64_t>(no); slot_off = dev.add<int32_t>(n_slots + 1); slot_obs = dev.add<int32_t>(no);
        obs_cam = dev.add<int32_t>(no); caminfo = dev.add<int32_t>((size_t)n_cams * 4);
        slot_desc = dev.add<int64_t>(no); obs_owner = dev.add<int8_t>(no);
        all_obs = dev.add<int32_t>(merged ? no : 0); slot_rec = dev.add<int64_t>(schurq ? ns * 2 : 0);
        for (int i = 0; i <= CCAL_MAX_CAMS; ++i) sorted[i] = dev.add<int32_t>(n_sorted[i]);
        h_gstatus = host.add<HostStatus, kCleared>(1); h_gstate = host.add<DevState>(1); h_pinned = host.add<double, kDoubles>(RB + 16);
    }
};

// poses a finishing single-launch group writes to the host with ALL its workgroups: up to 5 461 frames.  Stores of a shader cross the bus in
// 64-byte packets, the DMA engine's in 256+: 2 500 frames GN 0.150 -> 0.136 ms, 5 000: 0.184 -> 0.178, but 10 000: 0.238 -> 0.255 and, from a
// table sorted by corner count, scattered pose READS over the bus on top (0.219 -> 0.256): profiles/r06/ab_result_spread.txt
constexpr size_t kSpreadBytes = 256 * 1024;
// rows of the single-camera loop's partial-sum buffer = most wavefronts a Gram launch of this problem may have: one row per wavefront
// (fused elimination).  Up to 16 384 frames any lanes-per-frame mapping fits; beyond, the launchers keep to mappings that do - six
// lanes per frame (ten frames per wavefront) always does
inline int fused_partial_rows(int n_obs) {
    const int n_pw = std::max(std::min(std::max(n_obs, 1), 16384), (std::max(n_obs, 1) + 9) / 10 + 8);
    return (n_pw + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK * WAVES_PER_BLOCK;
}
struct FusedLayout {
    CallPlan dev, host;
    Slice<double> pf[2], praw[2], partial, red; Slice<int32_t> done_cnt;
    size_t red_stride = 0;                                      // doubles between red's two buffers
    Slice<double> mc_f, cost_f, d_stage;
    Slice<DevState> state;                                      // [0] the loops' state; [1], [2]: single-launch groups alternate
    Slice<HostStatus> h_status; Slice<double> h_result, h_stage;
    // PF, PRAW, RB1: pf_size, praw_size, fused_red_size of the problem's K; n_pw: fused_partial_rows
    FusedLayout(size_t n_slots, size_t n_obs, size_t PF, size_t PRAW, size_t RB1, size_t n_pw) {
        constexpr unsigned kCD = kCleared | kDoubles;
        const size_t ns = std::max<size_t>(n_slots, 1), no = std::max<size_t>(n_obs, 1);
        const size_t stage = std::max(ns * 6 + CCAL_PMAX + 8, RB1 + 8);       // the caller's [poses | intr] (+ 64 bytes); ccal_build_normal stages the reduced sums here
        for (auto& s : pf) s = dev.add<double, kCD>(ns * PF);
        for (auto& s : praw) s = dev.add<double, kCD>(no * PRAW);
        partial = dev.add<double, kCD>(RB1 * n_pw);
        red_stride = CallPlan::up256((RB1 + 7) * sizeof(double)) / sizeof(double);
        red = dev.add<double, kCD>(2 * red_stride); done_cnt = dev.add<int32_t, kCleared>(1);
        mc_f = dev.add<double, kDoubles>(no); cost_f = dev.add<double, kDoubles>(no);
        state = dev.add<DevState>(3); d_stage = dev.add<double, kDoubles>(stage);
        const bool zc = ns * 6 * sizeof(double) <= kSpreadBytes;     // (beyond kZeroCopyBytes: single-launch groups only, FusedJob::begin)
        h_status = host.add<HostStatus, kCleared>(1);
        h_result = host.add<double, kDoubles>(zc ? ns * 6 + CCAL_PMAX : 0); h_stage = host.add<double, kDoubles>(stage);
    }
};

// argument block of the per-slot elimination kernels (k_schur: ccal_kernels_normal.hip, k_schurq: ccal_kernels_schurq.hip)
struct SchurArgs {
    // the record buffers of parameter set 0 / 1 of the device-resident loop (host-driven form: [0] only).  An ARRAY indexed with
    // the set - one scalar load at a computed offset - and not `set == 1 ? G2 : G`: hipcc -O1 (ROCm 7.2) compiled that select
    // of two kernel-argument pointers behind `st != NULL && ...` into a branch that skips the load of G (every general solve
    // ended NOT_PD on records of zeros); at -O3 the same source happened to come out right - and stopped doing so when the
    // block grew by a pointer (the "136-byte" failures of this round).  Found with a -O1 host-sanitizer build
    const double* Gs[2];
    const int64_t* slot_desc;      // k_schur: per (slot, observation) in slot order: goff * 8 + camera - one load instead of three;
                                   // k_schurq: [n_slots][2] record offset (doubles) of camera 0 / 1 in the slot, -1 = none
    const int32_t* slot_off; const int32_t* caminfo; int32_t n_cams;
    int32_t n_slots, K, RB, PF, n_pw;
    int32_t STG;                   // per-wavefront staging (doubles) for record-format observations, 0 = none
    double lambda, min_diag, max_diag;
    double* partial; double* pf; const double* mc_slot;
    const DevState* st;                        // device-resident loop: Gram set and lambda come from the state
};

// the workspaces (ccal_solver_ws.hip)
void normal_ws_destroy(ccal_problem* p);
int normal_ws_ensure(ccal_problem* p);          // sizes, column table, camera step: allocate on first use
int normal_ws_ensure_general(ccal_problem* p);  // + the general (multi-camera) loop's buffers
__attribute__((visibility("hidden"))) int fused_ws_ensure(ccal_problem* p);           // + the single-camera loop's (after normal_ws_ensure)
int normal_upload_cols(ccal_problem* p);        // bounds / fixed flags -> device
// ccal_solver.hip: S [K][K], b [K], cost (any may be NULL) of the last ccal_build_normal_dev(p, lambda), in the caller's parameter
// order; waits for the stream.  CCAL_ERR_NOT_PD when a pose block failed in the elimination (ccal_build_normal, ccal_covariance)
int normal_readback(ccal_problem* p, double lambda, double* S, double* b, double* cost);
__attribute__((visibility("hidden"))) void build_cols(const ccal_problem* p, ColInfo* cols);        // [CCAL_KMAX]: the reduced system's columns, bounds and fixed flags in
__attribute__((visibility("hidden"))) void caller_columns(const ccal_problem* p, int* ext);         // [K]: reduced-system column -> the same parameter's column in the caller's order
// Session-sized solves (poses up to this many bytes: 2 048 frames) move their parameters without a copy operation: k_unpack1
// reads the caller's poses from pinned host memory, the k_head that finishes the solve writes the result there.  Larger
// problems stage through device copies (a kernel reading / writing half a megabyte across the bus one wavefront wide would
// cost more than the DMA it saves).
constexpr size_t kZeroCopyBytes = 96 * 1024;

// launchers (ccal_kernels_normal.hip).  Host-driven form: `cand` / gbuf / lambda select parameter set, G buffer and
// damping.  Device-resident form (st != NULL, *_dev): set 0 = (p->d_*, G[w->cur]), set 1 = (p->d_*_c, G[w->cur ^ 1]),
// the kernels pick the current set by st->cur, take lambda from st->lambda and do nothing once st->done is set.
#ifdef CCAL_LEGACY_KERNELS      // second library only (ccal_legacy_normal.hip): the matrix-core Gram, host-driven and device-resident form
hipError_t launch_gram(const ccal_problem* p, int cam, bool use_candidate_params, int gbuf, hipStream_t s);
hipError_t launch_gram_dev_mfma(const ccal_problem* p, int cam, const DevState* st, hipStream_t s);
#endif
hipError_t launch_gram_dev(const ccal_problem* p, int cam, const DevState* st, hipStream_t s);
hipError_t launch_gram_dev_all(const ccal_problem* p, const DevState* st, hipStream_t s);     // every camera: one launch if w->merged_gram, else one per camera
hipError_t launch_schur(const ccal_problem* p, int gbuf, double lambda, double min_diag, double max_diag, hipStream_t s,
                        const DevState* st = nullptr);
bool schurq_fits(int n_cams, const int* peff, const int* col_theta, const int* col_extr);      // ccal_kernels_schurq.hip
int schurq_slots_per_wave(int n_slots);         // 16 (four lanes per slot) or 8 (eight lanes per slot)
int schurq_rows(int n_slots, int slots_per_wave);
hipError_t launch_schurq(const SchurArgs& a, int peff, int rows, int slots_per_wave, hipStream_t s);
hipError_t launch_reduce(const ccal_problem* p, hipStream_t s, const DevState* st = nullptr);
hipError_t launch_solve(const ccal_problem* p, double lambda, double min_diag, double max_diag, hipStream_t s, DevState* st = nullptr,
                        HostStatus* hs = nullptr, int seq = 0, bool publish_all = false);
hipError_t launch_backsub(const ccal_problem* p, double lambda, double min_diag, double max_diag, hipStream_t s, const DevState* st = nullptr);
#ifdef CCAL_TEST_HOOKS          // second library only: k_solve / k_backsub as they are, device-resident form, on buffers of the tests' choice
// (ccal_test_camera_solve / ccal_test_backsub, ccal_legacy_test_hooks.hip).  Set 0 / 1 = intr[0], extr[0] / intr[1], extr[1]; damping and set from *st
struct TestSolveIO {
    const double* red; const ColInfo* cols; int32_t K; double min_diag, max_diag;
    double* intr[2]; double* extr[2]; int32_t n_intr, n_extr;
    double* dc; double* scal; int32_t* flags; DevState* st; HostStatus* hs;
};
struct TestBacksubIO {
    const double* pf; const double* dc; double* mc_slot; double* poses[2]; int32_t n_slots, K;
    double min_diag, max_diag; const DevState* st;
};
hipError_t test_launch_solve(const TestSolveIO& t, hipStream_t s);
hipError_t test_launch_backsub(const TestBacksubIO& t, hipStream_t s);
#endif

}  // namespace ccal

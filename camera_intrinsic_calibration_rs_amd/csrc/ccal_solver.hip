// Mode N host side: workspaces, ccal_build_normal and the optimizer loop (ccal_solve).
//
// The loop restates tiny_solver::GaussNewtonOptimizer::optimize as the reference calls it
// (src/util.rs:443-463, 668-670; defaults in ccal_set_defaults) -- per iteration: Jacobian at x,
// solve the normal equations, x <- clamp(x + dx), error(x), stop on min_error / |d error| thresholds --
// and adds a Ceres-style Levenberg-Marquardt mode on the same kernels.  Both loops (single camera: FusedJob, everything else:
// GeneralJob) are device-resident: the decisions run in a kernel, the host enqueues groups of launches one ahead and polls a
// status word in pinned memory.  The workspaces they run in: ccal_solver_ws.hip; several solves at once (ccal_solve_batch, the
// single-process sharded solve): ccal_solver_many.hip, through ccal_solver_job.hpp.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "ccal_solver_job.hpp"
#include "ccal_devopt.hpp"

using namespace ccal;

// HIP_TRY for enqueue(), which returns a sequence number: the status negated
#define HIP_TRYN(ctx, expr) HIP_TRY_RET(ctx, expr, -CCAL_ERR_HIP)


// gram (all cameras) at the current or candidate parameters into G[gbuf]
static int enqueue_gram(ccal_problem* p, bool cand, int gbuf) {
    ccal_ctx* ctx = p->ctx;
    NormalWs* w = p->nws;
    if (w->register_gram && !cand && gbuf == w->cur) {
        // record format (what k_schur expects): the device loop's launcher with the state set to "first evaluation of set 0"
        if (!w->gstate_is_eval) {      // as in the single-camera build: set once, valid until a solve rewrites the state
            HIP_TRY(ctx, launch_state_eval(w->d_gstate, 0.0, ctx->stream));
            w->gstate_is_eval = true;
        }
        HIP_TRY(ctx, launch_gram_dev_all(p, w->d_gstate, ctx->stream));
        return CCAL_OK;
    }
    if (w->register_gram) { ctx->err = "enqueue_gram: candidate sets go through the device loop"; return CCAL_ERR_UNSUPPORTED; }
#ifdef CCAL_LEGACY_KERNELS      // second library: the matrix-core pair (the product's normal_ws_ensure never plans a workspace without the register Gram)
    for (int c = 0; c < p->n_cams; ++c) HIP_TRY(ctx, launch_gram(p, c, cand, gbuf, ctx->stream));
    return CCAL_OK;
#else
    ctx->err = std::string("enqueue_gram: the matrix-core Gram: ") + hipGetErrorString(hipErrorNotSupported);
    return CCAL_ERR_HIP;
#endif
}

// The step's one collective: in-place sum of `n` doubles over the ranks, ordered on the context stream.  Native RCCL
// when a communicator is set (ccal_rccl.hip), else the callback, else nothing (single GPU).
static int allreduce(ccal_problem* p, double* buf, size_t n) {
    ccal_ctx* ctx = p->ctx;
    if (p->peer) { ctx->err = "this entry point does not run on a shard of an in-process device set (its sums are added by the solver's deciding kernel)"; return CCAL_ERR_UNSUPPORTED; }
    if (p->rccl_comm) return rccl_allreduce_sum(ctx, p->rccl_comm, buf, n, ctx->stream);
    if (p->allreduce && p->allreduce(p->allreduce_user, buf, n, (void*)ctx->stream) != 0) { ctx->err = "all-reduce callback failed"; return CCAL_ERR_HIP; }
    return CCAL_OK;
}

// schur + reduce (+ all-reduce) of G[gbuf] -> red
static int enqueue_reduce_system(ccal_problem* p, int gbuf, double lambda, double min_diag, double max_diag) {
    ccal_ctx* ctx = p->ctx;
    NormalWs* w = p->nws;
    HIP_TRY(ctx, launch_schur(p, gbuf, lambda, min_diag, max_diag, ctx->stream));
    HIP_TRY(ctx, launch_reduce(p, ctx->stream));
    return allreduce(p, w->red, (size_t)w->RB);
}

// Argument block of the single-camera kernels: set 0 = (p->d_intr, p->d_poses), set 1 = the *_c buffers.
static FusedArgs make_fused_args(const ccal_problem* p, double min_diag, double max_diag) {
    const NormalWs* w = p->nws;
    const FusedWs* f = w->fws;
    FusedArgs fa = {};
    fa.x = p->d_x; fa.y = p->d_y; fa.z = p->d_z; fa.u = p->d_u; fa.v = p->d_v;
    fa.obs_off = p->d_obs_off; fa.obs_slot = p->d_obs_slot; fa.slot_ident = p->slot_ident ? 1 : 0;
    fa.n_obs = p->n_obs; fa.K = p->K; fa.PF = w->PF; fa.PRAW = f->PRAW; fa.n_pw = f->n_pw;
    fa.fcbuf = f->fcbuf; fa.mc_f = f->mc_f; fa.cost_f = f->cost_f;
    fa.huber_delta = p->huber_delta; fa.min_diag = min_diag; fa.max_diag = max_diag; fa.rt = model_rt(p->ctx);
    fa.intr[0] = p->d_intr; fa.intr[1] = p->d_intr_c; fa.poses[0] = p->d_poses; fa.poses[1] = p->d_poses_c;
    fa.pf[0] = f->pf[0]; fa.pf[1] = f->pf[1]; fa.praw[0] = f->praw[0]; fa.praw[1] = f->praw[1];
    fa.dc = w->dc; fa.st = f->d_state; fa.partial = f->partial; fa.red = f->red;
    fa.avg_corners = (int32_t)(p->n_corners / std::max(p->n_obs, 1));
    fa.part_cap = f->n_pw;
    // ragged frames: the bins ccal_problem_create planned for the Gram launch (n_bins == 0: none)
    const GramBins& gb = p->gram_bins;
    fa.n_bins = (gb.n_bins > 0 && p->d_bin_tab) ? gb.n_bins : 0; fa.bin_tab = p->d_bin_tab;
    for (int b = 0; b < kGramMaxBins; ++b) { fa.bin_lpf[b] = gb.lpf[b]; fa.bin_first[b] = gb.first[b]; fa.bin_count[b] = gb.count[b]; fa.bin_wg0[b] = gb.wg0[b]; }
    fa.bin_wg0[kGramMaxBins] = gb.wg0[kGramMaxBins];
    return fa;
}
// Second library only: the separate elimination launch (k_schur1m, four frames per wavefront) fits the partial-sum buffer; sets fa.n_pw.
static bool fused_use_schur1m(const ccal_problem* p, FusedArgs& fa) {
    const int n_pw = (p->n_obs + 15) / 16 * 4;
    if (n_pw > p->nws->fws->n_pw) return false;
    fa.n_pw = n_pw;
    return true;
}
// Register-resident (VALU) Gram for every model: with the rotation columns in the phi basis it beats the matrix-core
// kernel also for the 120 / 136-entry triangles of OPENCV5 (10 000 frames, whole build: 70.0 vs 71.8 us two-focal, 59.9 vs
// 66.1 us one-focal; KB4 64.3 vs 74.0) - f64 MFMA shares the FP64 datapath with the VALU and a 16 x 16 tile computes
// 256 products where the triangle needs <= 136.  CCAL_GRAM=mfma selects the matrix-core kernel (k_gram1).
static bool fused_use_valu_gram(const ccal_problem* p) {
    (void)p;
#ifdef CCAL_LEGACY_KERNELS
    if (const char* g = dev_env("CCAL_GRAM")) return g[0] != 'm';
#endif
    return true;
}
// Gram + elimination of one group on the single-camera path (fa.n_part = the number of partial sums per entry)
static hipError_t enqueue_fused_gram_schur(const ccal_problem* p, FusedArgs& fa, bool schur_m, hipStream_t st) {
    fa.n_part = 0;
    if (p->n_obs <= 0) return hipSuccess;      // a rank whose shard is empty still takes part in the collective, with zeros
    // CCAL_FUSE_ELIM=0 (developer switch, read when the problem's workspace is created): always the separate elimination launch
    const bool valu = fused_use_valu_gram(p);
    fa.fuse_elim = (p->nws->fws->fuse_elim && valu) ? 1 : 0; fa.elim_fused = 0;
    // the matrix-core Gram (CCAL_GRAM=mfma) and the separate elimination launch (behind it, or CCAL_FUSE_ELIM=0) exist in the
    // second library only (ccal_legacy_fused.hip)
    hipError_t e = hipErrorNotSupported;
    if (valu) e = launch_gram1v(p->cams[0].model, p->one_focal, fa, st);
#ifdef CCAL_LEGACY_KERNELS
    else e = launch_gram1(p->cams[0].model, p->one_focal, fa, st);
#endif
    if (e != hipSuccess) return e;
    if (fa.elim_fused) return hipSuccess;      // the Gram kernel eliminated its frames' pose blocks itself: fa.n_part rows of partial sums
#ifdef CCAL_LEGACY_KERNELS
    if (schur_m) return launch_schur1m(fa, st);
#endif
    return hipErrorNotSupported;
}
// ... + k_reduce1: the reduced sums in fws->red (the all-reduce buffer of sharded solves; ccal_build_normal_dev)
static hipError_t enqueue_fused_system(const ccal_problem* p, FusedArgs& fa, bool schur_m, hipStream_t st) {
    if (hipError_t e = enqueue_fused_gram_schur(p, fa, schur_m, st); e != hipSuccess) return e;
    return launch_reduce1(fa, st);
}

// what a deciding kernel publishes of the state, written by the host (the word last, as the kernels do)
static void publish_state(HostStatus* hst, const DevState& ds, int seq) {
    hst->iter = ds.iter; hst->cur = ds.cur; hst->lm_accepted = ds.lm_accepted; hst->lm_rejected = ds.lm_rejected;
    hst->spec_hits = ds.spec_hits; hst->spec_misses = ds.spec_misses; hst->cur_cost = ds.cur_cost; hst->initial_cost = ds.initial_cost;
    hst->word = status_word(seq, ds.done, ds.done_seq);
}
// Host side of the device-resident loops: watch the status word a decision kernel publishes to pinned memory.
// One look, no blocking: *arrived = the step `target` has been published.  `since` = when the wait for this step began;
// timeout_s: seconds without the awaited step completing before the wait gives up; <= 0 = never (sharded solves: a late
// peer is waited for - an asymmetric give-up would leave the other ranks inside a collective with no partner).
// `spins` throttles the expensive checks (clock, stream query) to one in 4 096 looks.
int ccal::check_status(ccal_ctx* ctx, hipStream_t st, HostStatus* hst, const DevState* d_state, int target, double timeout_s,
                       std::chrono::steady_clock::time_point since, long* spins, bool* arrived) {
    *arrived = status_seq(hst->word) >= target;
    if (*arrived || (++*spins & 0xFFF) != 0) return CCAL_OK;
    const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - since).count();
    const hipError_t q = el > 0.002 ? hipStreamQuery(st) : hipErrorNotReady;
    if (q != hipSuccess && q != hipErrorNotReady) {      // the stream itself failed (a fault, a lost device): no step will ever publish
        ctx->err = std::string("device-resident solve: ") + hipGetErrorString(q);
        return CCAL_ERR_HIP;
    }
    if (q == hipSuccess && status_seq(hst->word) < target) {
        // stream drained but the word did not arrive: fall back to an explicit copy
        DevState ds;
        HIP_TRY(ctx, hipMemcpy(&ds, d_state, sizeof ds, hipMemcpyDeviceToHost));
        publish_state(hst, ds, target);
        *arrived = true;
        return CCAL_OK;
    }
    if (timeout_s > 0.0 && el > timeout_s) { ctx->err = "device-resident solve timed out"; return CCAL_ERR_HIP; }
    return CCAL_OK;
}

// Seconds WITHOUT A STEP COMPLETING before the host gives up.  Single GPU: 30.  Sharded: 600 - a peer that is still
// uploading or setting up its RCCL channels is waited for (a rank that gave up after 30 s left its peers inside a
// collective with no partner), but a peer that died must not hang the survivors for ever.
double ccal::wait_timeout(const ccal_problem* p, const ccal_solver_opts* o) {
    if (o->timeout_s > 0) return (double)o->timeout_s;
    return p->sharded() ? 600.0 : 30.0;
}
static void init_state(DevState* s, const ccal_solver_opts* o) {
    std::memset(s, 0, sizeof *s);
    const bool lm = o->method == CCAL_METHOD_LM;
    s->radius = o->lm_initial_radius; s->dec = 2.0;
    s->lambda = lm ? 1.0 / o->lm_initial_radius : 0.0;
    s->lambda_spec = lm ? 1.0 / lm_radius_cap(o->lm_initial_radius) : 0.0;
    s->min_error = o->min_error; s->min_abs = o->min_abs_error_decrease; s->min_rel = o->min_rel_error_decrease;
    s->cur = 0; s->first = 1; s->max_iter = o->max_iterations; s->method = o->method;
    s->error_metric = o->error_metric ? 1 : 0;
}
// Groups the host may enqueue at most: one per decision plus one re-elimination group per LM decision, plus the first.
static int max_groups_for(const ccal_solver_opts* o) {
    const int64_t n = (int64_t)(o->method == CCAL_METHOD_LM ? 2 : 1) * std::max(o->max_iterations, 0) + 2;
    return (int)std::min<int64_t>(n, kMaxGroups);      // sequence numbers travel in 24 bits of the status word
}
// How many groups are kept in flight ahead of the one the host waits for.  With native RCCL the collective is just
// another stream operation, so sharded solves run ahead like single-GPU ones; a callback is host code - the loop waits
// for every group before the next one (no collective is ever issued for a solve that has finished).
static int groups_in_flight(const ccal_problem* p, const char* env_name) {
    if (p->allreduce && !p->rccl_comm && !p->peer) {
        static const int hook_depth = std::max(1, dev_env_int("CCAL_FUSED_DEPTH_HOOK", 1));
        return hook_depth;
    }
    return std::max(1, dev_env_int(env_name, 2));
}

// ---------------------------------------------------------------------------------------------
// A solve as a resumable job: begin() stages the starting point and enqueues the first groups, poll() takes ONE look at
// the status word - consumes a published step, keeps `depth` groups in flight, reports when the solve has finished - and
// never blocks, end() fetches the result.  ccal_solve / ccal_solve_dev spin on poll(); ccal_solve_batch drives many jobs
// (each on its own context's stream) round-robin from one host thread, so that session-sized problems, which leave the
// GPU ~96 % idle one at a time, run side by side.
// Both loops are device-resident: accept / reject, damping, convergence tests and the camera solve run in a kernel.
// ---------------------------------------------------------------------------------------------
struct SolveJob {
    ccal_problem* p; const ccal_solver_opts* o; bool host_io;
    double* intr_io; double* poses_io; double* extr_io;
    ccal_ctx* ctx; NormalWs* w; hipStream_t st;
    std::chrono::steady_clock::time_point t0, t_wait;
    std::vector<int> pending;
    int enq = 0, max_groups = 0, depth = 1, seq = 0;
    long spins = 0;
    bool finished = false, enqueued_any = false;
    double timeout_s;                 // seconds without a step completing before the host gives up (wait_timeout)
    // single-process sharded solves: raised by the first shard that fails with something other than the solver's verdicts; its
    // peers - whose collectives will never find their partner - stop waiting at their next look instead of at the timeout
    const std::atomic<int>* cancel = nullptr;
    int share = 1;                    // ccal_solve_batch: problems solved side by side on this GPU (FusedArgs::share)
    SolveJob(ccal_problem* p_, const ccal_solver_opts* o_, bool hio, double* i, double* po, double* e)
        : p(p_), o(o_), host_io(hio), intr_io(i), poses_io(po), extr_io(e), ctx(p_->ctx), w(p_->nws), st(p_->ctx->stream), timeout_s(wait_timeout(p_, o_)) {}
    virtual ~SolveJob() {}
    virtual int begin() = 0;
    virtual int enqueue() = 0;                       // one group; returns its sequence number, < 0 on error
    virtual HostStatus* status() = 0;
    virtual const DevState* dev_state() = 0;
    virtual void mark_tail_pending() = 0;            // kernels are in flight that publish into the pinned status word
    virtual void swap_sets() = 0;                    // the accepted point lives in set 1: make it set 0 for whoever comes next
    virtual int fetch_result(hipStream_t dl, bool done) = 0;      // host_io: set 0 into the caller's arrays, downloads through dl
    hipStream_t side = nullptr;       // the workspace's side stream (set by begin())
    bool result_in_place = false;     // nothing of the result goes through a stream: on the host already, or it stays on the device
    int fail_enqueued(int code) { mark_tail_pending(); return code; }
    // The solve's epilogue.  `done` was published by the last instruction of the deciding kernel (after a system-scope fence):
    // everything the result depends on is complete.  A download goes through the side stream so that it does not queue behind the
    // early-exit groups still in the main stream; the next solve drains those before it starts.  A finished solve with nothing to
    // download does not wait for the stream either: the launch that said `done` has nothing left to write, and whatever runs next
    // on this stream is ordered behind it.
    int end(ccal_report* rep) {
        HostStatus* hst = status();
        hipStream_t dl = st;
        if (status_done(hst->word) && (!pending.empty() || result_in_place)) { dl = side; mark_tail_pending(); }
        else HIP_TRY(ctx, hipStreamSynchronize(st));
        const int done = status_done(hst->word);
        const int status = done ? done - 1 : CCAL_ERR_NO_CONVERGENCE;
        ccal_report R = {};
        R.status = status; R.iterations = hst->iter; R.lm_accepted = hst->lm_accepted; R.lm_rejected = hst->lm_rejected;
        R.lm_spec_hits = hst->spec_hits; R.lm_spec_misses = hst->spec_misses;
        R.initial_cost = hst->initial_cost; R.final_cost = hst->cur_cost;
        if (hst->cur == 1) swap_sets();
        if (host_io) {
            if (const int rc = fetch_result(dl, done != 0); rc != CCAL_OK) return rc;
            if (p->one_focal) for (int c = 0; c < p->n_cams; ++c) intr_io[c * CCAL_PMAX + 1] = intr_io[c * CCAL_PMAX];   // fy = f (src/util.rs:467-470)
        }
        R.solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (rep) *rep = R;
        if (status == CCAL_ERR_NOT_PD) ctx->err = "normal equations are not positive definite";
        return status;
    }
    // Sharded solves must issue the SAME sequence of collectives on every rank.  They do: every group carries exactly
    // one, the fill rule below is a function of the group that reported `done` only (groups enqueued = that index +
    // depth - 1, whatever the host timing), and `done` is decided from all-reduced sums, identically on every rank.
    int fill() {
        while ((int)pending.size() < depth && enq < max_groups) {
            const int sq = enqueue();
            if (sq < 0) return enqueued_any ? fail_enqueued(-sq) : -sq;
            enqueued_any = true;
            if (pending.empty()) t_wait = std::chrono::steady_clock::now();
            pending.push_back(sq); ++enq;
        }
        return CCAL_OK;
    }
    int poll(bool* fin) {
        *fin = finished;
        if (finished) return CCAL_OK;
        if (cancel && cancel->load(std::memory_order_acquire)) { ctx->err = "sharded solve: a peer shard failed"; return fail_enqueued(CCAL_ERR_HIP); }
        int rc = fill();
        if (rc != CCAL_OK) return rc;
        if (pending.empty()) { finished = true; *fin = true; return CCAL_OK; }
        const int waited = pending.front();
        bool arrived = false;
        HostStatus* hst = status();
        if ((rc = check_status(ctx, st, hst, dev_state(), waited, timeout_s, t_wait, &spins, &arrived)) != CCAL_OK) return fail_enqueued(rc);
        if (!arrived) return CCAL_OK;
        pending.erase(pending.begin());
        t_wait = std::chrono::steady_clock::now(); spins = 0;
        // act on `done` only when it was set by a step this thread has waited for: a later group may already have
        // published it, and how many groups get enqueued must not depend on that race (sharded ranks would issue
        // different numbers of collectives)
        const uint64_t wd = hst->word;
        if (status_done(wd) && status_done_seq(wd) <= waited) finished = true;
        else {
            if (o->verbose) std::printf("[ccal %s] iter %d cost %.12g\n", o->method == CCAL_METHOD_LM ? "LM" : "GN", hst->iter, hst->cur_cost);
            if ((rc = fill()) != CCAL_OK) return rc;
            if (pending.empty()) finished = true;
        }
        *fin = finished;
        return CCAL_OK;
    }
};

// Single-camera path: groups of (gram + elimination, reduce, [all-reduce], head), kernels of ccal_kernels_fused.hip /
// ccal_kernels_gram2.hip.  host_io: parameters come from / go back to the caller's host arrays (ccal_solve); otherwise they
// are and stay on the device (ccal_solve_dev).
struct FusedJob : SolveJob {
    FusedWs* f = nullptr;
    FusedArgs fa; HeadArgs ha; bool schur_m = false, sharded = false;
    // single-launch groups (k_gram1v<.., ITER>, IterArgs): launch s reads state buffer s & 1 and the rows of launch s - 1,
    // writes state buffer (s + 1) & 1 and its own rows into the other half of the partial-sum buffer
    int iter_rows = 0;
    bool batch_member = false;        // ccal_solve_batch drives this job's launches together with other problems' (run_iter_group): begin() enqueues nothing
    bool fold = false;                // the first single-launch group is also the solve's k_unpack1 (IterArgs::fold)
    UnpackArgs ua0;                   // its payload
    DevState* iter_state(int s) const { return f->d_state + 1 + (s & 1); }
    double* iter_partial(int s) const { return f->partial + (size_t)(s & 1) * iter_rows * f->RB1; }
    size_t np6 = 0;
    bool zero_copy = false;           // session-sized ccal_solve: poses read from / result written to pinned host memory by the kernels
    bool spread = false;              // zero_copy of a larger problem: every workgroup of the finishing single-launch group writes its slice of the poses
    void* pinned_dev = nullptr;       // large ccal_solve whose caller pinned poses_io (ccal_pin_buffer): its device-side address - no staging copy either way
    using SolveJob::SolveJob;
    HostStatus* status() override { return f->h_status; }
    const DevState* dev_state() override { return iter_rows ? iter_state(seq + 1) : f->d_state; }     // (read once the stream has drained)
    void mark_tail_pending() override { if (f) f->tail_pending = true; }
    int begin() override {
        int rc = fused_ws_ensure(p);
        if (rc != CCAL_OK) return rc;
        f = w->fws;
        const int K = p->K;
        t0 = std::chrono::steady_clock::now();
        // one pinned staging block [intr | state | cols | poses] -> ONE async copy -> k_unpack1 (both parameter sets start
        // from the same values; slots without observations never change).  ccal_solve_dev stages only the ~1 KB head.
        static_assert(sizeof(ColInfo) % 8 == 0, "ColInfo is staged as doubles");
        if ((rc = drain_tail(ctx, st, f->tail_pending)) != CCAL_OK) return rc;      // a stale k_head must not publish into this solve
        side = f->side;
        np6 = (size_t)p->n_slots * 6;
        fa = make_fused_args(p, o->lm_min_diagonal, o->lm_max_diagonal);
        sharded = p->sharded();
        fa.share = share;
        iter_rows = 0;
        if (!sharded && f->fuse_elim && fused_use_valu_gram(p)) {
            const int rows = fused_iter_rows(p->cams[0].model, p->one_focal, p->n_obs, fa.avg_corners, K, share, batch_member);
            if (rows > 0 && 2 * rows <= f->n_pw) iter_rows = rows;
        }
        // the result straight into pinned host memory: session sizes (one workgroup writes it: k_head or the single-launch group's
        // workgroup 0); larger problems only where EVERY workgroup of the finishing launch writes a slice (single-launch groups, not
        // the members of a lockstep batch).  CCAL_RESULT_SPREAD=0 (developer switch): the DMA behind the last launch.
        static const bool spread_off = dev_env_int("CCAL_RESULT_SPREAD", 1) == 0;
        const bool large = np6 * sizeof(double) > kZeroCopyBytes;
        spread = host_io && large && f->h_result != nullptr && iter_rows > 0 && !batch_member && !spread_off;
        zero_copy = host_io && f->h_result != nullptr && (!large || spread);
        result_in_place = zero_copy || !host_io;
        {
            // state, column table and intrinsics travel in k_unpack1's argument block; the poses are read in place from
            // pinned host memory (session sizes) or staged with one copy (large problems)
            UnpackArgs ua = {};
            init_state(&ua.st0, o);
            if (K > kFusedMaxK) { ctx->err = "single-camera loop: more than 9 camera columns"; return CCAL_ERR_INVALID_ARG; }
            ColInfo cols_all[CCAL_KMAX];
            build_cols(p, cols_all);
            for (int i = 0; i < K; ++i) ua.col0[i] = cols_all[i];
            ua.n_cols = K;
            ua.np6 = (int64_t)np6; ua.poses_on_device = host_io ? 0 : 1;
            ua.intr0 = p->d_intr; ua.intr1 = p->d_intr_c; ua.poses0 = p->d_poses; ua.poses1 = p->d_poses_c;
            ua.st = iter_rows ? iter_state(1) : f->d_state; ua.cols = w->cols;
            pinned_dev = (host_io && large && np6) ? pinned_device_ptr(poses_io, np6 * sizeof(double)) : nullptr;
            if (host_io) std::memcpy(ua.intr_h, intr_io, CCAL_PMAX * sizeof(double));
            // the caller's poses are pinned: k_unpack1 reads them where they are (no copy into the staging block, no DMA)
            if (host_io && pinned_dev) ua.poses_src = static_cast<const double*>(pinned_dev);
            else if (host_io) {
                std::memcpy(f->h_stage, poses_io, np6 * sizeof(double));
                if (zero_copy || np6 == 0) ua.poses_src = f->h_stage;
                else {
                    HIP_TRY(ctx, hipMemcpyAsync(f->d_stage, f->h_stage, np6 * sizeof(double), hipMemcpyHostToDevice, st));
                    ua.poses_src = f->d_stage;
                }
            }
            f->state_is_eval = false;
            // every slot observed (single camera: one frame per slot): the first single-launch group unpacks for itself - one launch
            // and the host's gap behind it less per solve.  CCAL_ITER_FOLD=0: k_unpack1.
            static const bool fold_off = dev_env_int("CCAL_ITER_FOLD", 1) == 0;
            if (f->all_slots_observed < 0) {
                std::vector<char> seen((size_t)std::max(p->n_slots, 1), 0);
                int n_seen = 0;
                for (int sl : p->h_obs_slot) if (sl >= 0 && sl < p->n_slots && !seen[(size_t)sl]) { seen[(size_t)sl] = 1; ++n_seen; }
                f->all_slots_observed = n_seen == p->n_slots ? 1 : 0;
            }
            fold = iter_rows > 0 && !fold_off && f->all_slots_observed == 1;
            ua0 = ua;                  // (fold: the first single-launch group's payload)
            if (!fold) HIP_TRY(ctx, launch_unpack1(ua, st));
        }
        enqueued_any = true;          // from here on an error exit leaves kernels in flight: the next solve / the destructor drains
        f->h_status->word = 0;
        schur_m = fused_use_schur1m(p, fa);
        ha = HeadArgs{};
        ha.st = f->d_state; ha.hs = f->h_status; ha.red = f->red; ha.cols = w->cols;
        ha.intr[0] = p->d_intr; ha.intr[1] = p->d_intr_c; ha.dc = w->dc; ha.K = K;
        ha.min_diag = o->lm_min_diagonal; ha.max_diag = o->lm_max_diagonal;
        ha.publish_all = o->verbose ? 1 : 0;
        ha.result_host = zero_copy ? f->h_result : nullptr;
        ha.poses[0] = p->d_poses; ha.poses[1] = p->d_poses_c; ha.np6 = (int64_t)np6;
        max_groups = max_groups_for(o) + (iter_rows ? 1 : 0);          // (single-launch groups: the decision on launch s is taken in launch s + 1)
        depth = groups_in_flight(p, "CCAL_FUSED_DEPTH");
        // single-launch groups publish their status word from the FRONT of the launch (the decision), ~10 us before the launch
        // ends: the host has the next launch in the stream in time without one enqueued ahead - and a finished solve leaves
        // no launches behind that exit early (each of which still sums the rows: four / eight sessions side by side 0.244 / 0.464
        // -> 0.236 / 0.444 ms per batch, one session 0.108 ms either way).  CCAL_FUSED_DEPTH overrides.
        if (iter_rows && !dev_env("CCAL_FUSED_DEPTH")) depth = 1;
        if (iter_rows) iter_args_common(fa.it);
        return batch_member ? CCAL_OK : fill();
    }
    // what every single-launch group of this solve finds in IterArgs (the per-launch fields are set by enqueue() / derived from the
    // launch number by k_gram1v_batch).  The payload of a folded first launch rides along in all of them: the kernels read it under
    // `fold` only.
    void iter_args_common(IterArgs& it) const {
        it.on = 1; it.publish_all = o->verbose ? 1 : 0; it.n_part_in = iter_rows;
        it.hs = f->h_status; it.cols = w->cols; it.dc_out = w->dc;
        it.result_host = zero_copy ? f->h_result : nullptr; it.np6 = (int64_t)np6;
        // (spread: never for a lockstep batch's members)
        it.result_poses = spread ? (pinned_dev ? static_cast<double*>(pinned_dev) : f->h_result + CCAL_PMAX) : nullptr;
        it.done_cnt = spread ? f->done_cnt : nullptr;
        it.n_cols = ua0.n_cols; it.poses_on_device = ua0.poses_on_device; it.poses_src = ua0.poses_src; it.cols_out = ua0.cols;
        it.st0 = ua0.st0;
        for (int i = 0; i < kFusedMaxK; ++i) it.col0[i] = ua0.col0[i];
        std::memcpy(it.intr_h, ua0.intr_h, sizeof it.intr_h);
    }
    // this problem's entry of a batch's table (k_gram1v_batch): bases instead of per-launch pointers
    FusedArgs batch_entry() const {
        FusedArgs e = fa;
        e.it.fold = fold ? 1 : 0; e.it.skip_head = 0; e.it.seq = 0;
        e.it.st_in = iter_state(0); e.it.st_out = nullptr; e.it.partial_in = nullptr;
        e.partial = f->partial; e.n_part = iter_rows; e.fuse_elim = 1; e.elim_fused = 1;
        return e;
    }
    int enqueue() override {          // one group: evaluation + elimination + ONE collective + decision/solve
        // CCAL_HEAD_REDUCE_ROWS=0 (developer switch): always the separate reduce launch
        static const int head_reduce_max_rows = std::min(dev_env_int("CCAL_HEAD_REDUCE_ROWS", kHeadReduceRows), kHeadReduceRows);
        if (iter_rows) {
            // session sizes on one GPU: the whole group is ONE launch - the Gram kernel sums the previous launch's rows, decides
            // and solves the camera system in front of its own evaluation (every workgroup the same arithmetic, workgroup 0 writes)
            const int sq = ++seq;
            IterArgs& it = fa.it;
            it.skip_head = sq == 1 ? 1 : 0; it.seq = sq; it.fold = (fold && sq == 1) ? 1 : 0;
            it.st_in = iter_state(sq); it.st_out = iter_state(sq + 1);
            it.partial_in = iter_partial(sq - 1); fa.partial = iter_partial(sq);
            HIP_TRYN(ctx, launch_gram_iter(p->cams[0].model, p->one_focal, fa, st));
            if (fa.n_part != iter_rows) { ctx->err = "single-launch group: row count changed"; return -CCAL_ERR_INVALID_ARG; }
            return sq;
        }
        if (sharded) {
            // Gram -> elimination -> reduce -> all-reduce of the packed sums -> head
            // in-process transport: the reduce leaves this rank's sums in one of two buffers, the head adds all ranks' (rank order)
            if (p->peer) fa.red = f->red + (size_t)inproc_parity(p->peer) * f->red_stride;
            HIP_TRYN(ctx, enqueue_fused_system(p, fa, schur_m, st));
            if (p->peer) {
                if (inproc_post(p->peer, fa.red, (size_t)f->RB1, (void*)st, &ha.peers) != 0) { ctx->err = "in-process transport: a peer shard failed or did not arrive"; return -CCAL_ERR_HIP; }
            } else if (int e = allreduce(p, f->red, (size_t)f->RB1); e != CCAL_OK) return -e;
            ha.partial = nullptr; ha.n_part = 0;
        } else {
            // single GPU: for session-sized problems (<= 40 rows of partial sums = 1 280 frames) the head adds them up itself,
            // three launches per group (600 / 1 000 frames: 23.6 / 24.4 -> 23.2 / 23.5 us per group); beyond ~3 000 frames one
            // workgroup reading all rows costs more than the reduce launch it replaces (10 000 frames: 58.6 vs 52.6 us).
            // Same sums bit for bit either way (reduce_partial_rows).
            HIP_TRYN(ctx, enqueue_fused_gram_schur(p, fa, schur_m, st));
            if (fa.n_part <= head_reduce_max_rows) { ha.partial = f->partial; ha.n_part = fa.n_part; }
            else { HIP_TRYN(ctx, launch_reduce1(fa, st)); ha.partial = nullptr; ha.n_part = 0; }
        }
        ha.seq = ++seq;
        HIP_TRYN(ctx, launch_head(ha, st));
        return seq;
    }
    void swap_sets() override { std::swap(p->d_intr, p->d_intr_c); std::swap(p->d_poses, p->d_poses_c); }
    int fetch_result(hipStream_t dl, bool done) override {
        if (zero_copy && done) {
            // the k_head that set `done` wrote the result into pinned memory before it published the word this thread
            // has just read: nothing to copy, nothing to wait for
            std::memcpy(intr_io, const_cast<const double*>(f->h_result), CCAL_PMAX * sizeof(double));
            if (!(spread && pinned_dev)) std::memcpy(poses_io, const_cast<const double*>(f->h_result) + CCAL_PMAX, np6 * sizeof(double));     // (pinned: written in place)
            return CCAL_OK;
        }
        // the caller's array is pinned: ONE DMA writes the poses where the caller reads them; else through the staging block
        double* h_to = pinned_dev ? poses_io : f->h_stage;
        double* h_intr = pinned_dev ? f->h_stage : f->h_stage + np6;
        if (np6) HIP_TRY(ctx, hipMemcpyAsync(h_to, p->d_poses, np6 * sizeof(double), hipMemcpyDeviceToHost, dl));
        HIP_TRY(ctx, hipMemcpyAsync(h_intr, p->d_intr, CCAL_PMAX * sizeof(double), hipMemcpyDeviceToHost, dl));
        HIP_TRY(ctx, hipStreamSynchronize(dl));
        if (!pinned_dev) std::memcpy(poses_io, f->h_stage, np6 * sizeof(double));
        std::memcpy(intr_io, h_intr, CCAL_PMAX * sizeof(double));
        return CCAL_OK;
    }
};

// General loop (several cameras, or CCAL_DISABLE_FUSED): the same group shape:
//   k_gram per camera at the evaluated set -> k_schur -> k_reduce -> (ONE all-reduce) -> k_solve (decision + camera
//   solve + candidate intrinsics / extrinsics) -> k_backsub (candidate poses, model decrease per slot)
// every kernel picks its parameter / Gram set and damping from the device state, k_solve applies the shared decision
// function and publishes a status word.  Set 0 = (p->d_*, G[w->cur]), set 1 = (p->d_*_c, G[w->cur ^ 1]).
struct GeneralJob : SolveJob {
    using SolveJob::SolveJob;
    HostStatus* status() override { return w->h_gstatus; }
    const DevState* dev_state() override { return w->d_gstate; }
    void mark_tail_pending() override { w->tail_pending = true; }
    int begin() override {
        int rc;
        if ((rc = normal_ws_ensure_general(p)) != CCAL_OK) return rc;
        if ((rc = drain_tail(ctx, st, w->tail_pending)) != CCAL_OK) return rc;      // a stale k_solve must not publish into this solve
        side = w->side;
        if (host_io && (rc = ccal_upload_params(p, intr_io, poses_io, extr_io)) != CCAL_OK) return rc;
        if ((rc = normal_upload_cols(p)) != CCAL_OK) return rc;
        w->peers.n = 0; w->red_out = nullptr;
        // the candidate poses are formed in the Gram kernels' prologue (one launch less per group: k_backsub).  Slots that no
        // frame observes are then never written: both parameter sets start from the same poses
        static const bool gbs_off = dev_env_int("CCAL_GEN_BACKSUB", 1) == 0;
        // (session-sized rigs: 600 slots x 2 / 3 cameras GN 0.229 / 0.277 -> 0.221 / 0.268 ms; at 2 x 10 000 frames the prologue's
        // extra work in 4 000 wavefronts costs more than the launch it saves - 0.459 against 0.440 ms - so: up to 4 000 frames)
        w->gen_backsub = w->register_gram && !gbs_off && p->n_obs <= 4000;
        w->lm_min_diag = o->lm_min_diagonal; w->lm_max_diag = o->lm_max_diagonal;
        if (w->gen_backsub && p->n_slots && !w->all_slots_observed)
            HIP_TRY(ctx, hipMemcpyAsync(p->d_poses_c, p->d_poses, sizeof(double) * p->n_slots * 6, hipMemcpyDeviceToDevice, st));
        t0 = std::chrono::steady_clock::now();
        w->gstate_is_eval = false;
        init_state(w->h_gstate, o);
        HIP_TRY(ctx, hipMemcpyAsync(w->d_gstate, w->h_gstate, sizeof(DevState), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemsetAsync(w->flags, 0, 4 * sizeof(int32_t), st));
        if (p->n_slots) HIP_TRY(ctx, hipMemsetAsync(w->mc_slot, 0, (size_t)p->n_slots * sizeof(double), st));
        w->h_gstatus->word = 0;
        enqueued_any = true;
        max_groups = max_groups_for(o);
        // sharded solves: every rank issues the same sequence of collectives - one per group, the decisions come from
        // all-reduced sums and the number of groups enqueued depends only on the group that reported `done`
        depth = groups_in_flight(p, "CCAL_GENERAL_DEPTH");
        return fill();
    }
    int enqueue() override {          // returns the sequence number that marks the group's end, < 0 on error
        const double min_d = o->lm_min_diagonal, max_d = o->lm_max_diagonal;
        DevState* ds = w->d_gstate;
        HIP_TRYN(ctx, launch_gram_dev_all(p, ds, st));
        HIP_TRYN(ctx, launch_schur(p, w->cur, 0.0, min_d, max_d, st, ds));
        if (p->peer) w->red_out = w->red + (size_t)inproc_parity(p->peer) * (size_t)(w->RB + 8);
        HIP_TRYN(ctx, launch_reduce(p, st, ds));
        if (p->peer) {
            const int bad = inproc_post(p->peer, w->red_out, (size_t)w->RB, (void*)st, &w->peers);
            w->red_out = nullptr;
            if (bad) { w->peers.n = 0; ctx->err = "in-process transport: a peer shard failed or did not arrive"; return -CCAL_ERR_HIP; }
        } else if (int e = allreduce(p, w->red, (size_t)w->RB); e != CCAL_OK) return -e;
        HIP_TRYN(ctx, launch_solve(p, 0.0, min_d, max_d, st, ds, w->h_gstatus, ++seq, o->verbose != 0));
        w->peers.n = 0;
        if (!w->gen_backsub) HIP_TRYN(ctx, launch_backsub(p, 0.0, min_d, max_d, st, ds));
        return seq;
    }
    void swap_sets() override {
        std::swap(p->d_intr, p->d_intr_c); std::swap(p->d_poses, p->d_poses_c); std::swap(p->d_extr, p->d_extr_c);
        w->cur ^= 1;
    }
    int fetch_result(hipStream_t dl, bool) override {
        HIP_TRY(ctx, hipMemcpyAsync(intr_io, p->d_intr, sizeof(double) * p->n_cams * CCAL_PMAX, hipMemcpyDeviceToHost, dl));
        if (poses_io && p->n_slots) HIP_TRY(ctx, hipMemcpyAsync(poses_io, p->d_poses, sizeof(double) * p->n_slots * 6, hipMemcpyDeviceToHost, dl));
        if (extr_io) HIP_TRY(ctx, hipMemcpyAsync(extr_io, p->d_extr, sizeof(double) * p->n_cams * 6, hipMemcpyDeviceToHost, dl));
        HIP_TRY(ctx, hipStreamSynchronize(dl));
        return CCAL_OK;
    }
};

// single camera: its own device-resident loop (GN and LM, sharded or not, empty shards included); the choice must not
// depend on anything rank-local, or sharded ranks would issue different collectives
static bool use_fused_path(const ccal_problem* p) { return p->n_cams == 1 && !dev_env("CCAL_DISABLE_FUSED"); }

int ccal::solve_entry(ccal_problem* p, const ccal_solver_opts* o, bool host_io, double* intr_io, double* poses_io, double* extr_io,
                      ccal_report* rep, const std::atomic<int>* cancel, int share) {
    ccal_ctx* ctx = p->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = normal_ws_ensure(p);
    if (rc != CCAL_OK) return rc;
    std::unique_ptr<SolveJob> job;
    if (use_fused_path(p)) job.reset(new FusedJob(p, o, host_io, intr_io, poses_io, extr_io));
    else job.reset(new GeneralJob(p, o, host_io, intr_io, poses_io, extr_io));
    job->cancel = cancel;
    job->share = share;
    if ((rc = job->begin()) != CCAL_OK) return rc;
    bool fin = false;
    while (!fin) if ((rc = job->poll(&fin)) != CCAL_OK) return rc;
    return job->end(rep);
}

// ---- a FusedJob as a member of a lockstep group (ccal_solver_job.hpp) ----------------------------------------------------------------
FusedJobPtr ccal::make_member(ccal_problem* p, const ccal_solver_opts* o, bool host_io, double* intr_io, double* poses_io) {
    return FusedJobPtr(new FusedJob(p, o, host_io, intr_io, poses_io, nullptr), [](FusedJob* j) { delete j; });
}
int ccal::prepare_member(FusedJob& j, hipStream_t st, int share) {
    ccal_problem* p = j.p;
    hipStream_t own = p->ctx->stream;
    // a stale launch of this problem's last solve may still sit in ITS OWN stream: the group's launches run elsewhere
    // (an error of this wait is left to the solve's own calls to report)
    if (p->nws->fws && own != st) (void)drain_tail(p->ctx, own, p->nws->fws->tail_pending);
    const bool fresh = !p->nws->fws;                     // begin() makes the workspace: its clears are ordered on the problem's own stream
    j.w = p->nws; j.st = st; j.share = share; j.batch_member = true;
    const int rc = j.begin();
    if (rc == CCAL_OK && fresh && own != st) HIP_TRY(p->ctx, hipStreamSynchronize(own));
    return rc;
}
bool ccal::fits(const FusedJob& j, int lpf) { return j.iter_rows > 0 && fused_iter_lpf(j.p->n_obs, j.fa.avg_corners, j.share) == lpf; }
int ccal::max_launches(const FusedJob& j) { return j.max_groups; }
FusedArgs ccal::batch_entry(const FusedJob& j) { return j.batch_entry(); }
int ccal::look(FusedJob& j, int s, std::chrono::steady_clock::time_point since, int label, bool* arrived, bool* done) {
    j.seq = s;
    *done = false;
    HostStatus* hst = j.f->h_status;
    const int rc = check_status(j.ctx, j.st, hst, j.dev_state(), s, j.timeout_s, since, &j.spins, arrived);
    if (rc != CCAL_OK || !*arrived) return rc;
    j.spins = 0;
    const uint64_t wd = hst->word;
    *done = status_done(wd) && status_done_seq(wd) <= s;
    if (!*done && j.o->verbose) std::printf("[ccal %s] problem %d iter %d cost %.12g\n", j.o->method == CCAL_METHOD_LM ? "LM" : "GN", label, hst->iter, hst->cur_cost);
    return CCAL_OK;
}
int ccal::finish(FusedJob& j, ccal_report* rep) {
    j.finished = true;
    const int rc = j.end(rep);
    j.f->tail_pending = false;          // (the group's stream has drained: nothing of this solve is left in flight)
    return rc;
}

extern "C" {

// developer hook of -DCCAL_STAMPS builds only (not part of include/ccal.h, not exported by the product build): copy the
// per-frame scratch of the fast path to the host; the diagnostic builds (tools/stamps_*.py) park in-kernel timestamps there
#ifdef CCAL_STAMPS
int ccal_debug_fcbuf(ccal_problem* p, double* out, int64_t n) {
    if (!p || !p->nws || !out) return CCAL_ERR_INVALID_ARG;
    if (!p->nws->fws) {          // general loop: what a -DCCAL_STAMPS build of k_schur4 leaves behind the partial sums
        const NormalWs* w = p->nws;
        if (!w->general_ready) return CCAL_OK;
        const int64_t room = (int64_t)w->RB * (std::max(w->n_pw, w->n_rows) - w->n_rows), m = std::min(n, room);
        if (m > 0 && hipMemcpy(out, w->partial + (int64_t)w->RB * w->n_rows, m * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return CCAL_ERR_HIP;
        return CCAL_OK;
    }
    const int64_t m = std::min<int64_t>(n, (int64_t)std::max(p->n_obs, 1) * 40);
    if (hipMemcpy(out, p->nws->fws->fcbuf, m * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return CCAL_ERR_HIP;
    return CCAL_OK;
}
#endif

int ccal_build_normal_dev(ccal_problem* p, double lambda) {
    if (!p) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    HIP_TRY(p->ctx, hipSetDevice(p->ctx->device));
    int rc = normal_ws_ensure(p);
    if (rc != CCAL_OK) return rc;
    NormalWs* w = p->nws;
    w->red_fused = false;
    if (use_fused_path(p) && p->n_obs > 0 && !p->sharded()) {
        // single camera: the device loop's own kernels (register / LDS Gram + per-frame elimination), evaluated at the
        // current parameters with the state set to "first evaluation"; fws->red = [A_dir | Y^T Y | . | failed blocks]
        ccal_ctx* ctx = p->ctx;
        if ((rc = fused_ws_ensure(p)) != CCAL_OK) return rc;
        FusedWs* f = w->fws;
        hipStream_t st = ctx->stream;
        if ((rc = drain_tail(ctx, st, f->tail_pending)) != CCAL_OK) return rc;
        FusedArgs fa = make_fused_args(p, 1e-6, 1e32);
        const bool schur_m = fused_use_schur1m(p, fa);
        // the device state only has to say "first evaluation of set 0 with this damping" - it still does after a build
        // (nothing decides), so back-to-back builds set it once; a solve invalidates the note
        if (!(f->state_is_eval && f->state_eval_lambda == lambda)) {
            HIP_TRY(ctx, launch_state_eval(f->d_state, lambda, st));
            f->state_is_eval = true; f->state_eval_lambda = lambda;
        }
        HIP_TRY(ctx, enqueue_fused_system(p, fa, schur_m, st));
        w->red_fused = true;
        return CCAL_OK;
    }
    if ((rc = normal_ws_ensure_general(p)) != CCAL_OK) return rc;
    if ((rc = drain_tail(p->ctx, p->ctx->stream, w->tail_pending)) != CCAL_OK) return rc;
    if ((rc = enqueue_gram(p, false, w->cur)) != CCAL_OK) return rc;
    return enqueue_reduce_system(p, w->cur, lambda, 1e-6, 1e32);
    CCAL_API_CATCH(p->ctx)
}

int ccal_build_normal(ccal_problem* p, const double* intr, const double* poses, const double* extr,
                      double lambda, double* S, double* b, double* cost) {
    if (!p || !intr || (!poses && p->n_slots) || (!extr && p->n_cams > 1)) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    int rc = ccal_upload_params(p, intr, poses, extr);
    if (rc != CCAL_OK) return rc;
    if ((rc = normal_ws_ensure(p)) != CCAL_OK) return rc;
    if ((rc = ccal_build_normal_dev(p, lambda)) != CCAL_OK) return rc;
    return normal_readback(p, lambda, S, b, cost);
    CCAL_API_CATCH(p->ctx)
}

}  // extern "C"
// what the last ccal_build_normal_dev(p, lambda) left on the device, in the caller's parameter order (waits for the stream)
int ccal::normal_readback(ccal_problem* p, double lambda, double* S, double* b, double* cost) {
    ccal_ctx* ctx = p->ctx;
    NormalWs* w = p->nws;
    const int K = w->K, K1 = K + 1;
    double failed = 0.0;
    int ec[CCAL_KMAX];
    caller_columns(p, ec);                   // S and b leave in the caller's parameter order
    // S(i, j) of the damped system and b = its column K, from the sums as the path at hand keeps them: at(i, j), j <= K, and the
    // diagonal the damping scales
    auto extract = [&](auto at, auto diag) {
        if (S) for (int i = 0; i < K; ++i) for (int j = 0; j < K; ++j) {
            double v = at(i, j);
            if (i == j && lambda > 0.0) v += lambda * std::min(std::max(diag(i), 1e-6), 1e32);
            S[ec[i] * K + ec[j]] = v;
        }
        if (b) for (int i = 0; i < K; ++i) b[ec[i]] = at(i, K);
    };
    const bool fused = w->red_fused;
    double* h = fused ? w->fws->h_stage : w->h_pinned;
    const size_t len = fused ? (size_t)w->fws->RB1 : (size_t)w->RB;
    HIP_TRY(ctx, hipMemcpyAsync(h, fused ? w->fws->red : w->red, len * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (fused) {
        // [A_dir | Y^T Y | . | failed]: S = A_dir - Y^T Y on the camera block, b its last column, cost = the r x r corner of A_dir
        const double* A = h; const double* Y = h + K1 * K1;
        extract([&](int i, int j) { return A[i * K1 + j] - Y[i * K1 + j]; }, [&](int i) { return A[i * K1 + i]; });
        if (cost) *cost = A[K * K1 + K];
        failed = h[2 * K1 * K1 + 1];
    } else {
        // the general path keeps the lower triangle of the (K + 1) x (K + 1) system (row K = b^T), the undamped diagonal behind it
        const double* hd = h + K1 * K1;
        extract([&](int i, int j) { return h[i >= j ? i * K1 + j : j * K1 + i]; }, [&](int i) { return hd[i]; });
        if (cost) *cost = h[w->RB - 3];
        failed = h[w->RB - 1];
    }
    if (failed > 0.0) { ctx->err = "a frame's pose block is not positive definite"; return CCAL_ERR_NOT_PD; }
    return CCAL_OK;
}
extern "C" {

int ccal_solve(ccal_problem* p, const ccal_solver_opts* o, double* intr_io, double* poses_io, double* extr_io, ccal_report* rep) {
    if (!p || !o || !intr_io || (!poses_io && p->n_slots) || (!extr_io && p->n_cams > 1)) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    return solve_entry(p, o, true, intr_io, poses_io, extr_io, rep);
    CCAL_API_CATCH(p->ctx)
}

int ccal_solve_dev(ccal_problem* p, const ccal_solver_opts* o, ccal_report* rep) {
    if (!p || !o) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    return solve_entry(p, o, false, nullptr, nullptr, nullptr, rep);
    CCAL_API_CATCH(p->ctx)
}

}  // extern "C"

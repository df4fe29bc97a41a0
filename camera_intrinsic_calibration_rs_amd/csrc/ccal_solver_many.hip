// Mode N host side, several solves at once: the contexts' persistent helper threads, ccal_solve_batch - independent problems side
// by side, session-sized single-camera ones in lockstep groups - and ONE problem sharded over the contexts of this process
// (ccal_solve_sharded; ccal_multi_solve goes through solve_sharded_run).  Every solve is the device-resident loop of
// ccal_solver.hip, reached through ccal_solver_job.hpp.
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ccal_solver_job.hpp"
#include "ccal_devopt.hpp"

using namespace ccal;

// A context's helper thread for ccal_solve_batch.  Persistent: a session-sized solve is ~0.15 ms, creating a thread per call
// costs a third of that (measured: four problems per call 1.35x over one at a time with threads made per call).  It spins for
// a short while after a task (the next batch usually follows at once), then sleeps on a condition variable.
struct ccal_ctx_worker {
    std::thread th;
    std::mutex m;
    std::condition_variable cv, cv_done;
    std::function<void()> task;
    std::atomic<int> has_task{0}, done{0}, stop{0};
    // how long a helper spins for its next task / the caller for a helper's result before either sleeps on its condition variable:
    // the next batch of session-sized solves usually follows within this window, a 50 000-frame upload does not - and must not
    // burn a core while it lasts
    static constexpr double kSpinSeconds = 100e-6;
    static bool spun_out(std::chrono::steady_clock::time_point t0, int spins) {
        return (spins & 0x3F) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > kSpinSeconds;
    }
    void loop() {
        for (;;) {
            int spins = 0;
            const auto t0 = std::chrono::steady_clock::now();
            while (!has_task.load(std::memory_order_acquire) && !stop.load(std::memory_order_acquire)) {
                if (!spun_out(t0, ++spins)) { cpu_relax(); continue; }
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return has_task.load() || stop.load(); });
            }
            if (stop.load()) return;
            task();
            has_task.store(0, std::memory_order_release);
            { std::lock_guard<std::mutex> lk(m); done.store(1, std::memory_order_release); }
            cv_done.notify_all();
        }
    }
    void submit(std::function<void()> fn) {
        { std::lock_guard<std::mutex> lk(m); task = std::move(fn); done.store(0); has_task.store(1, std::memory_order_release); }
        cv.notify_one();
    }
    // spin briefly (the helpers of a batch finish within microseconds of the caller's own solve), then sleep on the condition variable
    void wait() {
        const auto t0 = std::chrono::steady_clock::now();
        for (int spins = 1;; ++spins) { if (done.load(std::memory_order_acquire)) return; if (spun_out(t0, spins)) break; cpu_relax(); }
        std::unique_lock<std::mutex> lk(m);
        cv_done.wait(lk, [&] { return done.load(std::memory_order_acquire) != 0; });
    }
};
void ccal::ctx_worker_destroy(ccal_ctx* ctx) {
    ccal_ctx_worker* w = ctx->worker;
    if (!w) return;
    { std::lock_guard<std::mutex> lk(w->m); w->stop.store(1); }
    w->cv.notify_one();
    if (w->th.joinable()) w->th.join();
    delete w;
    ctx->worker = nullptr;
}
// The helper is published to the context only once its thread runs: if std::thread throws (EAGAIN) the context keeps no
// worker and the exception becomes the call's CCAL_ERR_HIP - a later call tries again instead of waiting on a thread
// that never existed.
void ccal::ctx_worker_submit(ccal_ctx* ctx, std::function<void()> fn) {
    if (!ctx->worker) {
        std::unique_ptr<ccal_ctx_worker> w(new ccal_ctx_worker());
        ccal_ctx_worker* raw = w.get();
        w->th = std::thread([raw] { raw->loop(); });
        ctx->worker = w.release();
    }
    ctx->worker->submit(std::move(fn));
}
void ccal::ctx_worker_wait(ccal_ctx* ctx) { if (ctx->worker) ctx->worker->wait(); }

// ---- ccal_solve_batch at session size: ONE launch per optimizer step for a whole group of problems ---------------------------
// A session-sized single-camera problem solved through single-launch groups costs the host four launches and their polls; n of
// them driven by n host threads were serialised by the runtime's launch path - eight 625-frame sessions took 0.48 ms per batch for
// ~0.1 ms of device work, whatever the kernels did.  Problems of one device, model, focal mode and lane mapping therefore advance in
// LOCKSTEP through k_gram1v_batch: launch s serves all of them (blockIdx.y = the problem; its argument block is an entry of a table
// written once per batch), the host waits for every member's word of launch s and enqueues launch s + 1 while any member is
// still running; a member that has finished leaves its later workgroups at their first look at the state.  Same arithmetic per
// problem as its own single-launch groups with this lane mapping: same verdicts, iteration counts, bits.
struct IterGroupKey { int device, model, one_focal, lpf; bool operator==(const IterGroupKey& o) const { return device == o.device && model == o.model && one_focal == o.one_focal && lpf == o.lpf; } };
// the lane mapping of the problem's single-launch groups when it is one of `share` problems side by side (0: that form does not apply)
static int batch_iter_lpf(const ccal_problem* p, int share) {
    if (p->n_cams != 1 || p->sharded() || p->n_obs <= 0 || p->K > kFusedMaxK || dev_env("CCAL_DISABLE_FUSED") || dev_env("CCAL_BATCH_LOCKSTEP_OFF")) return 0;
    const int avg = (int)(p->n_corners / std::max(p->n_obs, 1));
    const int rows = fused_iter_rows(p->cams[0].model, p->one_focal, p->n_obs, avg, p->K, share, true);
    if (rows <= 0 || 2 * rows > fused_partial_rows(p->n_obs)) return 0;
    return fused_iter_lpf(p->n_obs, avg, share);
}
// solve the members of one group; rc / reps per member.  Runs on the caller's thread.
// A member whose own preparation fails (workspace allocation, staging) takes its own code and error text and leaves the group; its
// neighbours go on (include/ccal.h: every problem's own verdict in reports[i]).  `retry`: members that are fine but do not fit this
// group after all - the caller solves them on their own.
static void run_iter_group(const IterGroupKey& key, const std::vector<int>& members_in, ccal_problem** ps, const ccal_solver_opts* o, bool host_io,
                           double** intr_io, double** poses_io, int share, std::vector<int>& rc, ccal_report* reps, std::vector<int>& retry) {
    std::vector<int> members;                                   // the members that made it into the launches
    ccal_ctx* c0 = ps[members_in[0]]->ctx;
    hipStream_t st = c0->stream;
    // failures of the GROUP (its device, its table): every member that is in the launches shares them
    auto fail_all = [&](const std::vector<int>& who, int code, const char* why) { for (int i : who) { rc[i] = code; note_error(ps[i]->ctx, why); } };
    if (hipSetDevice(c0->device) != hipSuccess) { fail_all(members_in, CCAL_ERR_HIP, "hipSetDevice failed"); return; }
    std::vector<FusedJobPtr> jobs;
    jobs.reserve(members_in.size());
    int max_rows = 0, max_groups = 0;
    for (int i : members_in) {
        ccal_problem* p = ps[i];
        int r = normal_ws_ensure(p);
#ifdef CCAL_TEST_HOOKS      // tests/test_gpu_iter.py (second library only): problem number CCAL_TEST_FAIL_BATCH_MEMBER of the batch fails its preparation
        if (const char* e = std::getenv("CCAL_TEST_FAIL_BATCH_MEMBER"); e && std::atoi(e) == i) { r = CCAL_ERR_NO_MEMORY; note_error(p->ctx, "injected failure of a batch member (test hook)"); }
#endif
        FusedJobPtr j = make_member(p, o, host_io, host_io ? intr_io[i] : nullptr, host_io && poses_io ? poses_io[i] : nullptr);
        if (r == CCAL_OK) {
            r = prepare_member(*j, st, share);
            if (r == CCAL_OK && !fits(*j, key.lpf)) {
                // prepared, but not in this group's shape after all: solved on its own behind the group (nothing of it was enqueued
                // on the group's stream but the staging, which its own solve repeats)
                (void)hipStreamSynchronize(st);
                retry.push_back(i);
                continue;
            }
        }
        if (r != CCAL_OK) { rc[i] = r; (void)hipStreamSynchronize(st); continue; }      // this member's own code; its context holds the reason
        max_groups = std::max(max_groups, max_launches(*j));
        jobs.push_back(std::move(j));
        members.push_back(i);
    }
    const int n = (int)members.size();
    if (n == 0) return;
    // the table: grown on demand, kept by the group's first context
    const size_t bytes = (size_t)n * sizeof(FusedArgs);
    if (c0->batch_tab_bytes < bytes) {
        ctx_release(c0, c0->d_batch_tab, false); ctx_release(c0, c0->h_batch_tab, true);      // (no launch of an earlier batch is left: each ends in a synchronise)
        c0->d_batch_tab = nullptr; c0->h_batch_tab = nullptr; c0->batch_tab_bytes = 0;
        const size_t want = std::max(bytes, (size_t)16 * sizeof(FusedArgs));
        if (ctx_dev_alloc(c0, (void**)&c0->d_batch_tab, want) != hipSuccess || ctx_host_alloc(c0, (void**)&c0->h_batch_tab, want) != hipSuccess) {
            (void)hipGetLastError(); fail_all(members, CCAL_ERR_NO_MEMORY, "ccal_solve_batch: out of memory for the batch table"); (void)hipStreamSynchronize(st); return;
        }
        c0->batch_tab_bytes = want;
    }
    FusedArgs* h_tab = reinterpret_cast<FusedArgs*>(c0->h_batch_tab);
    for (int k = 0; k < n; ++k) { h_tab[k] = batch_entry(*jobs[(size_t)k]); max_rows = std::max(max_rows, (int)h_tab[k].n_part); }
    bool ok = hipMemcpyAsync(c0->d_batch_tab, h_tab, bytes, hipMemcpyHostToDevice, st) == hipSuccess;
    std::vector<char> fin((size_t)n, 0);
    int n_fin = 0, err = CCAL_OK;
    for (int s = 1; ok && n_fin < n && s <= max_groups; ++s) {
        if (launch_gram_iter_batch(key.model, key.one_focal != 0, key.lpf, reinterpret_cast<const FusedArgs*>(c0->d_batch_tab), n, max_rows, s, st) != hipSuccess) { ok = false; break; }
        const auto t_wait = std::chrono::steady_clock::now();
        int arrived_n = n_fin;
        std::vector<char> got(fin);
        while (ok && arrived_n < n) {
            for (int k = 0; k < n; ++k) {
                if (got[(size_t)k]) continue;
                bool arrived = false, done = false;
                if ((err = look(*jobs[(size_t)k], s, t_wait, members[(size_t)k], &arrived, &done)) != CCAL_OK) { ok = false; break; }
                if (!arrived) continue;
                got[(size_t)k] = 1; ++arrived_n;
                if (done) { fin[(size_t)k] = 1; ++n_fin; }
            }
        }
    }
    // nothing of the group may still run when the members' buffers change hands (end() swaps parameter sets; the next solve of a
    // member may use its own stream)
    if (hipStreamSynchronize(st) != hipSuccess) ok = false;
    for (int k = 0; k < n; ++k) {
        const int i = members[(size_t)k];
        if (ok) rc[i] = finish(*jobs[(size_t)k], reps ? &reps[i] : nullptr);
        else { rc[i] = err != CCAL_OK ? err : CCAL_ERR_HIP; if (err == CCAL_OK) note_error(ps[i]->ctx, "ccal_solve_batch: a launch of the lockstep group failed"); }
    }
}

// Who drives what in one ccal_solve_batch call.  Session-sized single-camera problems of one device, model, focal mode and lane mapping
// advance in lockstep, one launch per step for the whole group (run_iter_group, on the caller's thread); everything else is driven per
// context: the problems of one context share its stream and are solved one after the other by one host thread.
namespace {
struct BatchPlan {
    std::vector<IterGroupKey> keys;               // the lockstep groups (two members and more), in order of first appearance,
    std::vector<std::vector<int>> members;        //   and their problems
    std::vector<char> grouped;                    // [n]: the problem is a member of one of them
    // the contexts that still have problems of their own: [0] is driven by the caller's thread - NULL when that thread has groups to
    // drive - the others by their helper threads
    std::vector<ccal_ctx*> ctxs;
    // ... but those that ALSO hold members of a group: driven on the caller's thread behind the groups - never by a helper thread while
    // the group's thread may write the same context's error text
    std::vector<ccal_ctx*> late;
};
}  // namespace
// how many of the batch's problems sit on the context's GPU: a problem's launches are sized for its share of that chip (FusedArgs::share)
static int side_by_side(ccal_problem* const* ps, int n, const ccal_ctx* c) { int k = 0; for (int i = 0; i < n; ++i) k += ps[i]->ctx->device == c->device ? 1 : 0; return k; }
static BatchPlan plan_batch(ccal_problem* const* ps, int n) {
    BatchPlan pl;
    pl.grouped.assign((size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        const int share = side_by_side(ps, n, ps[i]->ctx);
        const int lpf = share >= 2 ? batch_iter_lpf(ps[i], share) : 0;
        if (!lpf) continue;
        const IterGroupKey key = { ps[i]->ctx->device, ps[i]->cams[0].model, ps[i]->one_focal ? 1 : 0, lpf };
        size_t g = 0;
        while (g < pl.keys.size() && !(pl.keys[g] == key)) ++g;
        if (g == pl.keys.size()) { pl.keys.push_back(key); pl.members.emplace_back(); }
        pl.members[g].push_back(i);
    }
    for (size_t g = pl.keys.size(); g-- > 0;) {
        if (pl.members[g].size() < 2) { pl.keys.erase(pl.keys.begin() + (ptrdiff_t)g); pl.members.erase(pl.members.begin() + (ptrdiff_t)g); }
        else for (int i : pl.members[g]) pl.grouped[(size_t)i] = 1;
    }
    if (!pl.keys.empty()) pl.ctxs.push_back(nullptr);
    auto holds_grouped = [&](const ccal_ctx* c) { for (int i = 0; i < n; ++i) if (pl.grouped[(size_t)i] && ps[i]->ctx == c) return true; return false; };
    for (int i = 0; i < n; ++i) {
        if (pl.grouped[(size_t)i]) continue;
        std::vector<ccal_ctx*>& dst = holds_grouped(ps[i]->ctx) ? pl.late : pl.ctxs;
        if (std::find(dst.begin(), dst.end(), ps[i]->ctx) == dst.end()) dst.push_back(ps[i]->ctx);
    }
    return pl;
}

extern "C" {

// Several independent problems at once.  Every context with problems of its own is driven by its (persistent) helper thread, the
// first one by the caller's, so the contexts' streams are fed - a group is three to seven launches, ~10 us of host time, against
// ~35 us on the device for a session-sized problem: ONE thread feeding four streams is host-bound (measured: 1.3x over one problem
// at a time) - and their kernels overlap on the GPU.  Every problem's own verdict goes to its report; the return value is CCAL_OK
// unless a call failed for a reason other than the solver's verdicts (then the first such code, in problem order).
int ccal_solve_batch(ccal_problem** ps, int n, const ccal_solver_opts* o, double** intr_io, double** poses_io, double** extr_io,
                     ccal_report* reps) {
    if (!ps || n < 0 || !o) return CCAL_ERR_INVALID_ARG;
    for (int i = 0; i < n; ++i) {
        if (!ps[i]) return CCAL_ERR_INVALID_ARG;
        for (int k = 0; k < i; ++k) if (ps[k] == ps[i]) return CCAL_ERR_INVALID_ARG;
        if (intr_io && (!intr_io[i] || (!(poses_io && poses_io[i]) && ps[i]->n_slots) || (!(extr_io && extr_io[i]) && ps[i]->n_cams > 1))) return CCAL_ERR_INVALID_ARG;
        if (ps[i]->sharded()) { ps[i]->ctx->err = "ccal_solve_batch: sharded problems are solved one at a time (their collectives order the ranks)"; return CCAL_ERR_UNSUPPORTED; }
    }
    ccal_ctx* c0 = n ? ps[0]->ctx : nullptr;
    CCAL_API_TRY
    const bool host_io = intr_io != nullptr;
    std::vector<int> rc(n, CCAL_ERR_HIP);
    BatchPlan pl = plan_batch(ps, n);
    // a problem that ended without the solver's verdict: its report says so
    auto settle = [&](int i) { if (reps && rc[i] != CCAL_OK && rc[i] != reps[i].status) blank_report(&reps[i], rc[i]); };
    auto run_ctx = [&](ccal_ctx* c) noexcept {
        const int n_side = side_by_side(ps, n, c);
        for (int i = 0; i < n; ++i) {
            if (ps[i]->ctx != c || pl.grouped[(size_t)i]) continue;
            rc[i] = guarded(c, "C++ exception in ccal_solve_batch", [&] {
                return solve_entry(ps[i], o, host_io, host_io ? intr_io[i] : nullptr, host_io && poses_io ? poses_io[i] : nullptr,
                                   host_io && extr_io ? extr_io[i] : nullptr, reps ? &reps[i] : nullptr, nullptr, n_side);
            });
            settle(i);
        }
    };
    auto drive_here = [&] {
        if (pl.keys.empty()) { if (!pl.ctxs.empty()) run_ctx(pl.ctxs[0]); return; }
        for (size_t g = 0; g < pl.keys.size(); ++g) {
            const std::vector<int>& mem = pl.members[g];
            std::vector<int> retry;                    // members sent back: solved on their own, behind the groups
            const int grc = guarded(nullptr, "", [&] { run_iter_group(pl.keys[g], mem, ps, o, host_io, intr_io, poses_io, side_by_side(ps, n, ps[mem[0]]->ctx), rc, reps, retry); return (int)CCAL_OK; });
            if (grc != CCAL_OK) for (int i : mem) rc[i] = grc;
            for (int i : retry) { pl.grouped[(size_t)i] = 0; if (std::find(pl.late.begin(), pl.late.end(), ps[i]->ctx) == pl.late.end()) pl.late.push_back(ps[i]->ctx); }
            for (int i : mem) if (pl.grouped[(size_t)i]) settle(i);
        }
        for (ccal_ctx* c : pl.late) run_ctx(c);
    };
    ctx_fan_out(pl.ctxs.data(), (int)pl.ctxs.size(), [&](int k) { run_ctx(pl.ctxs[(size_t)k]); }, drive_here, [] {});
    for (int i = 0; i < n; ++i)
        if (rc[i] == CCAL_ERR_HIP || rc[i] == CCAL_ERR_INVALID_ARG || rc[i] == CCAL_ERR_NO_MEMORY || rc[i] == CCAL_ERR_UNSUPPORTED) return rc[i];
    return CCAL_OK;
    CCAL_API_CATCH(c0)
}

}  // extern "C"

// ---- ONE problem whose frame slots are sharded over n contexts of THIS process (include/ccal.h) --------------------
// Every shard is driven by a host thread of its own - the caller's thread takes shard 0, the contexts' persistent helper
// threads the others - exactly like the ranks of a multi-process run: each thread runs the ordinary device-resident loop
// on its shard and issues the step's collective on its context's stream (native RCCL: one communicator per device made
// by ncclCommInitAll; or a stream-ordered callback transport).  The decisions are functions of all-reduced sums only, so
// every shard ends with the same status, iteration count and - bit for bit - the same camera block.
static bool verdict(int rc) { return rc == CCAL_OK || rc == CCAL_ERR_NONFINITE || rc == CCAL_ERR_NOT_PD || rc == CCAL_ERR_NO_CONVERGENCE; }
int ccal::solve_sharded_run(ccal_problem** ps, int n, const ccal_solver_opts* o, double* intr_io, double* const* poses_io, double* extr_io,
                      ccal_report* rep, InprocComm* inproc) {
    const int n_cams = ps[0]->n_cams;
    const size_t ni = (size_t)n_cams * CCAL_PMAX, ne = (size_t)n_cams * 6;
    std::vector<double> intr((size_t)n * ni), extr((size_t)n * ne, 0.0);
    for (int i = 0; i < n; ++i) {
        std::memcpy(&intr[i * ni], intr_io, ni * sizeof(double));
        if (extr_io) std::memcpy(&extr[i * ne], extr_io, ne * sizeof(double));
    }
    std::vector<int> rc((size_t)n, CCAL_ERR_HIP);
    std::vector<ccal_report> reps((size_t)n);
    // fault injection for tests/test_gpu_multi.py - in builds with -DCCAL_TEST_HOOKS only (libccal_hip_legacy.so, which the product
    // never loads): CCAL_TEST_FAIL_SHARD=r makes shard r fail before it enqueues anything - its peers are then inside the step's
    // collective with no partner, which is what the transport's abort / timeout path is for
#ifdef CCAL_TEST_HOOKS
    const int fail_shard = [] { const char* e = std::getenv("CCAL_TEST_FAIL_SHARD"); return e ? std::atoi(e) : -1; }();
#else
    constexpr int fail_shard = -1;
#endif
    std::atomic<int> cancel{0}, first_failed{-1};        // first_failed: the shard that raised `cancel` (its peers fail BECAUSE of it)
    auto run = [&](int i) noexcept {
        if (i == fail_shard) { rc[i] = CCAL_ERR_HIP; note_error(ps[i]->ctx, "injected failure (test hook)"); }
        else rc[i] = guarded(ps[i]->ctx, "C++ exception in ccal_solve_sharded", [&] {
            return solve_entry(ps[i], o, true, &intr[i * ni], poses_io ? poses_io[i] : nullptr, &extr[i * ne], &reps[i], &cancel);
        });
        if (!verdict(rc[i])) {
            // this shard has left the shared sequence of collectives: its peers must not wait for it - neither in the in-process
            // transport's host barrier nor, with RCCL, for a step whose ncclAllReduce will never find its partner (the caller
            // aborts the communicators once every thread is back)
            int none = 0;
            if (cancel.compare_exchange_strong(none, 1, std::memory_order_acq_rel)) first_failed.store(i, std::memory_order_release);
            if (inproc) inproc_abort(inproc);
        }
    };
    std::vector<ccal_ctx*> ctxs((size_t)n);
    for (int i = 0; i < n; ++i) ctxs[(size_t)i] = ps[i]->ctx;
    // (a helper thread that could not be made: the ranks already started wait for the missing one - the transport lets them go)
    ctx_fan_out(ctxs.data(), n, run, [&] { run(0); }, [&] { if (inproc) inproc_abort(inproc); });
    // the shard that failed FIRST is the one to report (its peers then gave up with "a peer shard failed")
    int first_bad = first_failed.load(std::memory_order_acquire);
    for (int i = 0; i < n && first_bad < 0; ++i) if (!verdict(rc[i])) first_bad = i;
    if (first_bad >= 0) {
        if (first_bad != 0) note_error(ps[0]->ctx, (std::string("shard ") + std::to_string(first_bad) + ": " + ps[first_bad]->ctx->err).c_str());
        blank_report(rep, rc[first_bad]);
        return rc[first_bad];
    }
    // one decision sequence, one camera block: anything else is a defect of the transport (sums that differ between ranks)
    for (int i = 1; i < n; ++i) {
        if (rc[i] != rc[0] || reps[i].iterations != reps[0].iterations ||
            std::memcmp(&intr[i * ni], &intr[0], ni * sizeof(double)) != 0 || std::memcmp(&extr[i * ne], &extr[0], ne * sizeof(double)) != 0) {
            note_error(ps[0]->ctx, "ccal_solve_sharded: the shards disagree on the result (transport defect)");
            blank_report(rep, CCAL_ERR_HIP);
            return CCAL_ERR_HIP;
        }
    }
    std::memcpy(intr_io, &intr[0], ni * sizeof(double));
    if (extr_io) std::memcpy(extr_io, &extr[0], ne * sizeof(double));
    if (rep) {
        *rep = reps[0];
        for (int i = 1; i < n; ++i) rep->solve_ms = std::max(rep->solve_ms, reps[i].solve_ms);
    }
    return rc[0];
}

extern "C" {

int ccal_solve_sharded(ccal_problem** ps, int n, const ccal_solver_opts* o, double* intr_io, double** poses_io, double* extr_io,
                       ccal_report* rep) {
    if (!ps || n < 1 || !o || !intr_io) return CCAL_ERR_INVALID_ARG;
    for (int i = 0; i < n; ++i) if (!ps[i]) return CCAL_ERR_INVALID_ARG;
    ccal_ctx* c0 = ps[0]->ctx;
    CCAL_API_TRY
    int n_native = 0, n_cb = 0, n_peer = 0;
    for (int i = 0; i < n; ++i) {
        const ccal_problem* p = ps[i];
        if ((p->n_slots && !(poses_io && poses_io[i])) || (p->n_cams > 1 && !extr_io)) { c0->err = "ccal_solve_sharded: null parameter array"; return CCAL_ERR_INVALID_ARG; }
        for (int k = 0; k < i; ++k) if (ps[k]->ctx == p->ctx) { c0->err = "ccal_solve_sharded: every shard needs a context of its own (one host thread and one stream per shard)"; return CCAL_ERR_INVALID_ARG; }
        if (p->n_cams != ps[0]->n_cams || p->K != ps[0]->K || p->one_focal != ps[0]->one_focal || p->huber_delta != ps[0]->huber_delta) { c0->err = "ccal_solve_sharded: the shards describe different problems"; return CCAL_ERR_INVALID_ARG; }
        for (int c = 0; c < p->n_cams; ++c) if (p->cams[c].model != ps[0]->cams[c].model) { c0->err = "ccal_solve_sharded: the shards describe different cameras"; return CCAL_ERR_INVALID_ARG; }
        if (std::memcmp(p->lo.data(), ps[0]->lo.data(), p->lo.size() * sizeof(double)) || std::memcmp(p->hi.data(), ps[0]->hi.data(), p->hi.size() * sizeof(double)) ||
            p->has_bound != ps[0]->has_bound || p->fixed != ps[0]->fixed) { c0->err = "ccal_solve_sharded: the shards carry different bounds / fixed parameters"; return CCAL_ERR_INVALID_ARG; }
        n_native += p->rccl_comm ? 1 : 0; n_cb += (!p->rccl_comm && p->allreduce) ? 1 : 0; n_peer += p->peer ? 1 : 0;
    }
    if (n == 1 && !ps[0]->sharded()) return solve_entry(ps[0], o, true, intr_io, poses_io ? poses_io[0] : nullptr, extr_io, rep);
    if ((n_native && n_native != n) || (n_cb && n_cb != n) || (n_peer && n_peer != n) || (n_native > 0) + (n_cb > 0) + (n_peer > 0) > 1) { c0->err = "ccal_solve_sharded: a transport on some shards only"; return CCAL_ERR_INVALID_ARG; }
    if (n_peer) { c0->err = "ccal_solve_sharded: the shards of a ccal_multi_problem are solved by ccal_multi_solve"; return CCAL_ERR_INVALID_ARG; }
    if (n_native || n_cb) return solve_sharded_run(ps, n, o, intr_io, poses_io, extr_io, rep, nullptr);
    // no transport set: the library's own in-process one for the duration of the call (shards on one GPU, or on GPUs with
    // peer access); ccal_multi_* keeps a transport - RCCL when the devices differ - for the lifetime of the device set
    std::vector<int> devs((size_t)n);
    for (int i = 0; i < n; ++i) devs[i] = ps[i]->ctx->device;
    std::string err;
    InprocComm* ic = inproc_create(n, devs.data(), &err);
    if (!ic) { c0->err = "ccal_solve_sharded: " + err; return CCAL_ERR_UNSUPPORTED; }
    for (int i = 0; i < n; ++i) ps[i]->peer = inproc_rank_handle(ic, i);
    inproc_set_timeout(ic, wait_timeout(ps[0], o));
    int rc = CCAL_ERR_HIP;
    try { rc = solve_sharded_run(ps, n, o, intr_io, poses_io, extr_io, rep, ic); } catch (...) { rc = CCAL_ERR_NO_MEMORY; }
    // the early-exit groups enqueued ahead reference the transport's events and buffers: drain them before it goes
    for (int i = 0; i < n; ++i) {
        bool queued = true;                    // whatever the workspaces' flags say: a solve that left by an exception set none
        (void)hipSetDevice(ps[i]->ctx->device);
        (void)drain_tail(ps[i]->ctx, ps[i]->ctx->stream, queued);
        if (ps[i]->nws) { ps[i]->nws->tail_pending = false; if (ps[i]->nws->fws) ps[i]->nws->fws->tail_pending = false; }
        ps[i]->peer = nullptr;
    }
    inproc_destroy(ic);
    return rc;
    CCAL_API_CATCH(c0)
}

}  // extern "C"

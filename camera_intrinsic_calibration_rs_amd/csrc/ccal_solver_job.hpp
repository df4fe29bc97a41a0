// What ccal_solver_many.hip - several solves at once: ccal_solve_batch and the single-process sharded solve - needs of the
// device-resident loops in ccal_solver.hip.  Private to those two units: no kernel unit includes it.
#pragma once
#include <atomic>
#include <chrono>
#include <memory>

#include "ccal_fused.hpp"

struct FusedJob;                 // the single-camera loop (ccal_solver.hip)

#pragma GCC visibility push(hidden)      // between two units of one library
namespace ccal {

// one whole solve on the calling thread.  cancel: raised by a peer shard that failed (the sharded solve); share: how many problems
// of the call run side by side on this GPU (FusedArgs::share)
int solve_entry(ccal_problem* p, const ccal_solver_opts* o, bool host_io, double* intr_io, double* poses_io, double* extr_io,
                ccal_report* rep, const std::atomic<int>* cancel = nullptr, int share = 1);
// seconds WITHOUT A STEP COMPLETING before the host gives up
double wait_timeout(const ccal_problem* p, const ccal_solver_opts* o);
// one look at a status word, no blocking: *arrived = the step `target` has been published
int check_status(ccal_ctx* ctx, hipStream_t st, HostStatus* hst, const DevState* d_state, int target, double timeout_s,
                 std::chrono::steady_clock::time_point since, long* spins, bool* arrived);

// A single-camera solve as a member of a lockstep group (run_iter_group): the group owns the launches - one k_gram1v_batch per step
// for all members, on the group's stream - the member stages its starting point, reads its own status word and fetches its own result.
using FusedJobPtr = std::unique_ptr<FusedJob, void (*)(FusedJob*)>;
FusedJobPtr make_member(ccal_problem* p, const ccal_solver_opts* o, bool host_io, double* intr_io, double* poses_io);
// stage the starting point on the group's stream `st` as one of `share` problems side by side; enqueues no group.  What the problem's
// last solve left in its own stream is waited for, and so are the clears of a workspace made here (they run on the problem's stream).
int prepare_member(FusedJob& j, hipStream_t st, int share);
bool fits(const FusedJob& j, int lpf);            // single-launch groups with this lane mapping: the member can join the group's launches
int max_launches(const FusedJob& j);              // launches the solve may take at most
FusedArgs batch_entry(const FusedJob& j);         // the member's entry of the group's table: bases instead of per-launch pointers; n_part = its rows
// one look at the member's word of launch s (`since`: when the group began to wait for it).  *arrived: published; *done: the solve has
// finished with a step up to s.  `label`: the problem's number in the call, for verbose output.
int look(FusedJob& j, int s, std::chrono::steady_clock::time_point since, int label, bool* arrived, bool* done);
// the group's stream has drained: the member's verdict, report and result
int finish(FusedJob& j, ccal_report* rep);

}  // namespace ccal
#pragma GCC visibility pop

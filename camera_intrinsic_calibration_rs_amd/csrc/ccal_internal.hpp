// Host-side structures shared by the API translation unit and the kernel launchers.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstring>
#include <exception>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ccal.h"
#include "ccal_models.hpp"
#include "ccal_plan.hpp"

namespace ccal {

constexpr int WAVES_PER_BLOCK = 4;     // 256 threads: one wavefront per observation frame
constexpr int PF_STRIDE = 64;          // doubles kept per frame slot for back-substitution

// Arguments of the per-camera kernels (everything device-resident).
struct KArgs {
    const float* x; const float* y; const float* z; const float* u; const float* v;
    const int64_t* obs_off;        // [n_obs+1]
    const int32_t* obs_slot;       // [n_obs]
    const int64_t* joff;           // [n_obs] offset (doubles) of the frame's block Jacobians in J_out
    const int32_t* list;           // observation frames of this camera
    int32_t n_list;
    int32_t cam;
    const double* intr;            // [n_cams][CCAL_PMAX] full params
    const double* poses;           // [n_slots][6]
    const double* extr;            // [n_cams][6]
    double huber_delta;
    ModelRt rt;                    // the context's run-time conventions (KB4 threshold, OPENCV5 coefficient order)
    int32_t apply_loss;
    double* r_out;                 // mode E
    double* J_out;
    double* err_out;               // reprojection errors
};

struct NormalWs;

struct CamLayout {
    int model = 0, P = 0, Peff = 0, D = 0;
    int col_theta = 0, col_extr = -1;
    double width = 0, height = 0;
    std::vector<int32_t> obs;          // host copy of the camera's observation frames
    int32_t* d_obs = nullptr;
};

}  // namespace ccal

struct ccal_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    ccal_model_conventions conv;   // run-time model conventions (defaults: ccal_models.hpp)
    // a problem holds its context: ccal_ctx_destroy with problems still alive only marks it, the last
    // ccal_problem_destroy frees it (bindings with a garbage collector destroy in any order)
    int n_problems = 0;
    bool destroy_requested = false;
    // ccal_solve_batch: the host thread that drives this context's stream while the caller's thread drives another one
    // (created on first use, joined when the context is freed; ccal_solver_many.hip)
    struct ccal_ctx_worker* worker = nullptr;
    // ccal_solve_batch, session sizes: the argument blocks of a batch's problems, one launch per step for all of them
    // (k_gram1v_batch reads the table on the device; h_: its pinned staging) - blocks of the context's allocator, grown on demand, released with the context
    char* d_batch_tab = nullptr; char* h_batch_tab = nullptr; size_t batch_tab_bytes = 0;
    // ccal_pin_buffer: the caller's ranges this context registered (unregistered by ccal_unpin_buffer or with the context)
    std::vector<std::pair<void*, size_t>> pinned;
    // Blocks of device and pinned host memory (and side streams) that destroyed problems of this context gave back: a calibration
    // session creates a problem per camera and per retry (src/bin/camera_calibration.rs:205-265) - hipMalloc / hipHostMalloc /
    // hipStreamCreate and their frees were a third of a 600-frame session's create + first solve.  A few blocks, bounded sizes;
    // freed with the context.  `live`: what is handed out (pointer -> bytes, second = 1 for pinned host memory).
    struct Block { void* p; size_t bytes; };
    std::vector<Block> cache_dev, cache_host;
    std::vector<hipStream_t> cache_streams;
    std::vector<std::pair<void*, std::pair<size_t, int>>> live;
};
namespace ccal {
constexpr size_t kCacheDevMaxBytes = (size_t)1 << 30, kCacheHostMaxBytes = (size_t)64 << 20;
constexpr size_t kCacheMaxBlocks = 12;
// a block of at least `bytes` (256-byte granularity): from the context's cache when one fits without wasting more than a quarter
inline hipError_t ctx_alloc(ccal_ctx* ctx, void** out, size_t bytes, bool host, unsigned host_flags = 0) {
    bytes = (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255;
    std::vector<ccal_ctx::Block>& cache = host ? ctx->cache_host : ctx->cache_dev;
    size_t best = cache.size();
    for (size_t i = 0; i < cache.size(); ++i)
        if (cache[i].bytes >= bytes && cache[i].bytes <= bytes + bytes / 4 + 4096 && (best == cache.size() || cache[i].bytes < cache[best].bytes)) best = i;
    void* p = nullptr;
    size_t got = bytes;
    if (best != cache.size()) { p = cache[best].p; got = cache[best].bytes; cache.erase(cache.begin() + (ptrdiff_t)best); }
    else {
        const hipError_t e = host ? hipHostMalloc(&p, bytes, host_flags) : hipMalloc(&p, bytes);
        if (e != hipSuccess) return e;
    }
    try { ctx->live.emplace_back(p, std::make_pair(got, host ? 1 : 0)); }
    catch (...) { if (host) (void)hipHostFree(p); else (void)hipFree(p); throw; }
    *out = p;
    return hipSuccess;
}
inline hipError_t ctx_dev_alloc(ccal_ctx* ctx, void** out, size_t bytes) { return ctx_alloc(ctx, out, bytes, false); }
// pinned, mapped, coherent host memory (every pinned block of the library is allocated that way: one kind in the cache)
inline hipError_t ctx_host_alloc(ccal_ctx* ctx, void** out, size_t bytes) { return ctx_alloc(ctx, out, bytes, true, hipHostMallocCoherent | hipHostMallocMapped); }
// give a block back (anything not handed out by ctx_alloc - or with no context left - is simply freed).  The caller has made sure
// nothing in flight still uses it.
inline void ctx_release(ccal_ctx* ctx, void* p, bool host) {
    if (!p) return;
    if (ctx) {
        for (size_t i = 0; i < ctx->live.size(); ++i) {
            if (ctx->live[i].first != p) continue;
            const size_t bytes = ctx->live[i].second.first;
            const bool is_host = ctx->live[i].second.second != 0;
            ctx->live.erase(ctx->live.begin() + (ptrdiff_t)i);
            std::vector<ccal_ctx::Block>& cache = is_host ? ctx->cache_host : ctx->cache_dev;
            size_t total = bytes;
            for (const auto& b : cache) total += b.bytes;
            if (!ctx->destroy_requested && cache.size() < kCacheMaxBlocks && total <= (is_host ? kCacheHostMaxBytes : kCacheDevMaxBytes)) {
                try { cache.push_back({ p, bytes }); return; } catch (...) { }
            }
            if (is_host) (void)hipHostFree(p); else (void)hipFree(p);
            return;
        }
    }
    if (host) (void)hipHostFree(p); else (void)hipFree(p);
}
inline hipError_t ctx_stream_get(ccal_ctx* ctx, hipStream_t* out) {
    if (!ctx->cache_streams.empty()) { *out = ctx->cache_streams.back(); ctx->cache_streams.pop_back(); return hipSuccess; }
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}
inline void ctx_stream_put(ccal_ctx* ctx, hipStream_t s) {
    if (!s) return;
    if (ctx && !ctx->destroy_requested && ctx->cache_streams.size() < 4) { try { ctx->cache_streams.push_back(s); return; } catch (...) { } }
    (void)hipStreamDestroy(s);
}
// Test hook of the second library (-DCCAL_TEST_HOOKS): with CCAL_TEST_POISON_ALLOC=1 fill a freshly allocated (or cache-reused) block
// of DOUBLES with 0xFF bytes - a quiet NaN - before the library's own clears and uploads, so that a result depending on memory nobody
// wrote turns into NaN (tests/test_gpu_poison.py).  Never called on indices, offsets, counters, flags or DevState.  Defined out of
// line in ccal_solver_ws.hip, which each library compiles itself; hidden, so that each library calls its own.  The product's is empty.
__attribute__((visibility("hidden"))) hipError_t test_poison_f64(ccal_ctx* ctx, void* p, size_t bytes, bool host, hipStream_t s);
// Test hook of the second library, the same way: true with CCAL_TEST_GUARD_SLICES=1 - a one-shot call's block (ccal_call.hpp:
// CallBlock) then keeps a guard of a known byte in front of its first slice and behind every slice, and finish() reports a damaged one
// (tests/test_gpu_guard.py).  Read on every call.  The product's returns false.
__attribute__((visibility("hidden"))) bool test_guard_slices();
// A persistent block as its plan describes it: from the context's allocator, the test hook's NaN over its slices of doubles, then ONE
// clear of the slices that must start as zeros - on the context's stream (it does not synchronise with the null stream), in front of every use
inline hipError_t ctx_block_alloc(ccal_ctx* ctx, const CallPlan& pl, char** out, bool host) {
    hipError_t e = host ? ctx_host_alloc(ctx, (void**)out, pl.total) : ctx_dev_alloc(ctx, (void**)out, pl.total);
    for (int i = 0; i < pl.n_poison && e == hipSuccess; ++i) e = test_poison_f64(ctx, *out + pl.poison[i].off, pl.poison[i].bytes, host, ctx->stream);
    if (e != hipSuccess || !pl.zero_bytes) return e;
    if (host) { std::memset(*out, 0, pl.zero_bytes); return hipSuccess; }
    return hipMemsetAsync(*out, 0, pl.zero_bytes, ctx->stream);
}
// a buffer of n doubles made on first use, which the library writes before it reads (*out != NULL: there already)
inline hipError_t ctx_doubles(ccal_ctx* ctx, double** out, size_t n) {
    if (*out) return hipSuccess;
    const hipError_t e = ctx_dev_alloc(ctx, (void**)out, n * sizeof(double));
    return e != hipSuccess ? e : test_poison_f64(ctx, *out, n * sizeof(double), false, ctx->stream);
}
inline void ctx_cache_clear(ccal_ctx* ctx) {
    for (auto& b : ctx->cache_dev) (void)hipFree(b.p);
    for (auto& b : ctx->cache_host) (void)hipHostFree(b.p);
    for (hipStream_t s : ctx->cache_streams) (void)hipStreamDestroy(s);
    ctx->cache_dev.clear(); ctx->cache_host.clear(); ctx->cache_streams.clear();
}
}  // namespace ccal
namespace ccal {
// The device-side address of caller memory that is pinned (registered with ccal_pin_buffer / hipHostRegister, or allocated with
// hipHostMalloc) for all of [host, host + bytes); nullptr: ordinary pageable memory - the library stages it.
inline void* pinned_device_ptr(const void* host, size_t bytes) {
    if (!host || !bytes) return nullptr;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, host) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (at.type != hipMemoryTypeHost || !at.devicePointer) return nullptr;
    hipPointerAttribute_t at2;                     // the range's last byte lies in the same registration
    if (hipPointerGetAttributes(&at2, static_cast<const char*>(host) + bytes - 1) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (at2.type != hipMemoryTypeHost || !at2.devicePointer ||
        static_cast<char*>(at2.devicePointer) - static_cast<char*>(at.devicePointer) != (ptrdiff_t)(bytes - 1)) return nullptr;
    return at.devicePointer;
}
}  // namespace ccal
namespace ccal {
void ctx_worker_destroy(ccal_ctx* ctx);
// ccal_api.hip: an object other than a problem that was counted in ctx->n_problems (an undistortion map) lets go of its context
void ctx_unref(ccal_ctx* ctx);
// the context's conventions as the kernels take them
inline ModelRt model_rt(const ccal_ctx* ctx) {
    ModelRt rt = {};
    rt.kb4_eps = ctx->conv.kb4_small_radius; rt.unproject_eps = ctx->conv.unproject_small_radius;
    rt.ocv5_perm = 0;
    for (int i = 0; i < 5; ++i) rt.ocv5_perm |= (uint32_t)(ctx->conv.ocv5_order[i] & 7) << (3 * i);
    return rt;
}
inline bool ocv5_identity(const ccal_ctx* ctx) { return model_rt(ctx).ocv5_perm == kOcv5IdentityPerm; }
}  // namespace ccal

namespace ccal {
// Ragged single-camera problems: the bins of a Gram launch (gram2_bin_plan, ccal_kernels_gram2.hip).  Bin b: bin_count[b] frames - positions
// bin_first[b] .. of the problem's table of frames sorted by corner count - with bin_lpf[b] lanes per frame, worked on by the
// workgroups bin_wg0[b] .. bin_wg0[b + 1] - 1 of ONE launch.
constexpr int kGramMaxBins = 5;
struct GramBins {
    int32_t n_bins = 0;               // 0: no bins (every frame the same lanes per frame, frames in table order)
    int32_t lpf[kGramMaxBins] = {}, first[kGramMaxBins] = {}, count[kGramMaxBins] = {}, wg0[kGramMaxBins + 1] = {};
    int32_t fold = 0;                 // > 0: ONE bin, the table folded at this position (frames behind it smallest first)
};
// The plan for corner counts n[0 .. n_obs) (host): which frames go together and with how many lanes each; order = the sorted table
// (frame indices, bins in launch order).  n_bins == 0: binning does not pay (uniform frames, too few of them).
GramBins gram2_bin_plan(const int64_t* obs_off, int n_obs, bool two_per_simd, std::vector<int32_t>* order, bool rig_list = false);

// ccal_problem::d_block: the corner arrays, the frame tables and each camera's list of frames (one element of slack behind each: the
// Gram / eval kernels request a frame's first corner row before they look at its corner count - for an EMPTY last frame one past the
// data), the sorted table of ragged single-camera problems, then the two parameter sets, which start as zeros behind [0, uploaded)
struct ProblemLayout {
    CallPlan plan;
    Slice<float> x, y, z, u, v; Slice<int64_t> obs_off, joff;
    Slice<int32_t> obs_cam, obs_slot, cam_obs[CCAL_MAX_CAMS], bin_tab;
    size_t uploaded = 0;
    Slice<double> intr, poses, extr, intr_c, poses_c, extr_c;
    ProblemLayout(size_t n_corners, size_t n_obs, size_t n_slots, int n_cams, const size_t* n_cam_obs, size_t n_bin_tab) {
        for (Slice<float>* s : { &x, &y, &z, &u, &v }) *s = plan.add<float>(n_corners + 1);
        obs_off = plan.add<int64_t>(n_obs + 2); joff = plan.add<int64_t>(n_obs + 2);
        obs_cam = plan.add<int32_t>(n_obs + 1); obs_slot = plan.add<int32_t>(n_obs + 1);
        for (int c = 0; c < n_cams; ++c) cam_obs[c] = plan.add<int32_t>(n_cam_obs[c] + 1);
        bin_tab = plan.add<int32_t>(n_bin_tab ? n_bin_tab + 1 : 0);
        uploaded = plan.total;
        const size_t ni = (size_t)n_cams * CCAL_PMAX, np6 = std::max<size_t>(n_slots, 1) * 6, ne = (size_t)n_cams * 6;
        intr = plan.add<double>(ni); poses = plan.add<double>(np6); extr = plan.add<double>(ne);
        intr_c = plan.add<double>(ni); poses_c = plan.add<double>(np6); extr_c = plan.add<double>(ne);
    }
};

}  // namespace ccal

struct ccal_problem {
    ccal_ctx* ctx = nullptr;
    int n_cams = 0, n_slots = 0, n_obs = 0, K = 0;
    bool one_focal = false;
    double huber_delta = 1.0;
    int64_t n_corners = 0, j_len = 0;
    std::vector<ccal::CamLayout> cams;
    std::vector<int64_t> h_obs_off, h_joff;
    std::vector<int32_t> h_obs_cam, h_obs_slot;
    bool slot_ident = false;       // h_obs_slot[o] == o for every observation frame
    bool has_nonplanar = false;    // some corner has z != 0: pose initialisation also launches the general PnP (ccal_kernels_pnp.hip)
    // single camera, ragged frames: the bins of the Gram launch and the sorted table int4 { frame, first corner, corners, slot } per
    // position (a slice of d_block); gram_bins.n_bins == 0: none
    ccal::GramBins gram_bins;
    int32_t* d_bin_tab = nullptr;
    // device-resident inputs
    char* d_scratch = nullptr; size_t scratch_bytes = 0;      // validation()'s temporaries (grown on demand, kept between calls)
    char* d_block = nullptr;       // ONE device allocation: the corner arrays, the frame tables and the six parameter arrays are slices of it
    float *d_x = nullptr, *d_y = nullptr, *d_z = nullptr, *d_u = nullptr, *d_v = nullptr;
    int64_t *d_obs_off = nullptr, *d_joff = nullptr;
    int32_t *d_obs_cam = nullptr, *d_obs_slot = nullptr;
    // device-resident parameters (current point and candidate)
    double *d_intr = nullptr, *d_poses = nullptr, *d_extr = nullptr;
    double *d_intr_c = nullptr, *d_poses_c = nullptr, *d_extr_c = nullptr;
    // constraints in eff index space [n_cams][CCAL_PMAX]
    std::vector<double> lo, hi;
    std::vector<uint8_t> has_bound, fixed;
    // mode N / solver workspaces (allocated lazily)
    ccal::NormalWs* nws = nullptr;
    // lazily sized scratch for host<->device staging of ccal_eval
    double *d_r = nullptr, *d_J = nullptr, *d_err = nullptr;
    char* d_cov = nullptr;                     // ccal_covariance's block (CovLayout), made at the first call
    ccal_allreduce_fn allreduce = nullptr;     // callback form of the step's collective (tests over gloo)
    void* allreduce_user = nullptr;
    void* rccl_comm = nullptr;                 // ncclComm_t: the library issues ncclAllReduce itself (ccal_set_rccl_comm)
    void* peer = nullptr;                      // the library's in-process transport (ccal_multi.hip, an InprocRank): the deciding kernel
                                               // adds the ranks' buffers itself; stream-ordered, groups are enqueued ahead like with RCCL
    bool counted = false;                      // registered in ctx->n_problems (creation succeeded)
    bool sharded() const { return allreduce != nullptr || rccl_comm != nullptr || peer != nullptr; }
};

// No exception crosses the C ABI (include/ccal.h:9): every extern "C" body that can allocate host memory (operator new,
// std::vector, std::string) runs between CCAL_API_TRY and CCAL_API_CATCH(ctx).  ctx may be NULL.
#define CCAL_API_TRY try {
#define CCAL_API_CATCH(ctx_expr)                                                                   \
    }                                                                                              \
    catch (const std::bad_alloc&) { ccal::note_error((ctx_expr), "out of host memory"); return CCAL_ERR_NO_MEMORY; }  \
    catch (const std::exception& e_) { ccal::note_error((ctx_expr), e_.what()); return CCAL_ERR_HIP; }                \
    catch (...) { ccal::note_error((ctx_expr), "unknown C++ exception"); return CCAL_ERR_HIP; }

// A HIP call of a function that returns a ccal_status: on failure the context's message is "<the call>: <HIP's text>" and the
// function returns CCAL_ERR_HIP (HIP_TRY_RET: `ret`, for a function whose return value carries something else as well).
#define HIP_TRY_RET(ctx, expr, ret)                                                                \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                        \
            return ret;                                                                            \
        }                                                                                          \
    } while (0)
#define HIP_TRY(ctx, expr) HIP_TRY_RET(ctx, expr, CCAL_ERR_HIP)

namespace ccal {
inline void note_error(ccal_ctx* ctx, const char* msg) noexcept {
    if (!ctx) return;
    try { ctx->err = msg; } catch (...) { }
}
inline void note_error(const ccal_ctx*, const char*) noexcept {}
// model id check shared by the entry points that take one camera model (or one per camera): CCAL_OK, or the status with the message set
inline int check_model(ccal_ctx* ctx, int model, const char* where) {
    const bool eucmt = model == CCAL_MODEL_EUCMT;
    if (!eucmt && model >= 0 && model < kNumModels) return CCAL_OK;
    try {
        ctx->err = std::string(where) + (eucmt ? ": EUCMT is a parameter container in this build (its projection is only in the absent camera-intrinsic-model crate)"
                                               : ": unknown camera model");
    } catch (...) { }
    return eucmt ? CCAL_ERR_UNSUPPORTED : CCAL_ERR_INVALID_ARG;
}
// caller's params() vector -> th[CCAL_PMAX] in the kernels' canonical order (OPENCV5: k1, k2, p1, p2, k3, permuted here from
// ccal_model_conventions.ocv5_order; the rest 0) and the conventions of kernels that take their parameters that way
inline void canonical_theta(const ccal_ctx* ctx, int model, const double* params, double* th, ModelRt* rt) {
    for (int i = 0; i < CCAL_PMAX; ++i) th[i] = 0.0;
    for (int i = 0; i < model_np(model); ++i) th[i] = params[(model == kOCV5 && i >= 4) ? 4 + ctx->conv.ocv5_order[i - 4] : i];
    *rt = model_rt(ctx);
    rt->ocv5_perm = kOcv5IdentityPerm;
}
// the host's switch on a (checked) model id: Launch<MODEL>::go(grid, stream, args) launches the kernel's instance
template <template <int> class Launch, class Args>
void launch_model(int model, int grid, hipStream_t st, const Args& a) {
    switch (model) {
        case kUCM: Launch<kUCM>::go(grid, st, a); break;
        case kEUCM: Launch<kEUCM>::go(grid, st, a); break;
        case kKB4: Launch<kKB4>::go(grid, st, a); break;
        default: Launch<kOCV5>::go(grid, st, a); break;
    }
}
// kernel launchers (ccal_kernels.hip)
hipError_t launch_eval(const ccal_problem* p, int cam, const KArgs& a, hipStream_t s);
hipError_t launch_reproj_err(const ccal_problem* p, int cam, const KArgs& a, hipStream_t s);
// ccal_rccl.hip: in-place sum over the ranks of an ncclComm_t, ordered on the stream; returns a ccal_status
int rccl_allreduce_sum(ccal_ctx* ctx, void* comm, double* buf, size_t count, hipStream_t st);
// A finished solve may leave early-exit groups in its stream (`flag`: a workspace's tail_pending); they publish into the workspace's
// pinned status word, so whoever uses it next waits for them first.  No-op when the flag is down.
__attribute__((visibility("hidden"))) inline int drain_tail(ccal_ctx* ctx, hipStream_t st, bool& flag) {
    if (!flag) return CCAL_OK;
    HIP_TRY(ctx, hipStreamSynchronize(st));
    flag = false;
    return CCAL_OK;
}
// ccal_solver_ws.hip: the same for both workspaces of a problem, on its context's stream
int drain_pending_groups(ccal_problem* p);
// ccal_kernels_stats.hip
// ccal_problem::d_scratch, grown on demand and kept between calls, as its two users cut it:
//   ccal_init_poses       poses [n_obs][6] | counts [n_obs]
//   validation()          offsets [frames of the camera + 1] | values [n] | the selection's work area
// (the multi-GPU form's block - order_stats_block, ccal_multi.hip - is the second without offsets: the values in front)
constexpr size_t kSelWorkBytes = 103680;           // sizeof(SelWork) rounded up (ccal_kernels_stats.hip asserts it)
struct PoseScratch {
    CallPlan plan; Slice<double> poses; Slice<int32_t> counts;
    explicit PoseScratch(size_t n_obs) { poses = plan.add<double, kDoubles>(std::max<size_t>(n_obs, 1) * 6); counts = plan.add<int32_t>(std::max<size_t>(n_obs, 1)); }
};
struct StatsScratch {
    CallPlan plan; Slice<int64_t> offsets; Slice<double> values; Slice<char> work;
    StatsScratch(size_t n_offsets, int64_t n) { offsets = plan.add<int64_t>(n_offsets); values = plan.add<double, kDoubles>((size_t)n); work = plan.add<char>(kSelWorkBytes); }
};
// ccal_problem::d_cov, ccal_covariance's block (ccal_kernels_cov.hip), made at the first call and kept: the per-frame records
// { V_o (21) | W_o (15 x 6, rows past the camera's columns 0) | sum r^2 }, S^-1 (zero rows and columns at fixed parameters),
// the per-corner leverages, the two sums (+ 128 partial sums behind them), the slots' 6 x 6 blocks; then the slot -> observation frames table and the slots' verdicts
constexpr int kCovCamCols = 15;                                  // camera columns of one block at most: 9 intrinsics + 6 extrinsics
constexpr int kCovRec = 21 + 6 * kCovCamCols + 1;                // doubles per record
struct CovLayout {
    CallPlan plan; Slice<double> rec, sinv, lev, sums, pose_cov; Slice<int32_t> slot_off, slot_obs, status;
    CovLayout(size_t n_corners, size_t n_obs, size_t n_slots, size_t K) {
        const size_t no = std::max<size_t>(n_obs, 1), ns = std::max<size_t>(n_slots, 1);
        rec = plan.add<double, kDoubles>(no * kCovRec); sinv = plan.add<double, kDoubles>(std::max<size_t>(K * K, 1));
        lev = plan.add<double, kDoubles>(std::max<size_t>(n_corners, 1)); sums = plan.add<double, kDoubles>(8 + 128);
        pose_cov = plan.add<double, kDoubles>(ns * 36);
        slot_off = plan.add<int32_t>(n_slots + 1); slot_obs = plan.add<int32_t>(no); status = plan.add<int32_t>(ns);
    }
};
// first size of ccal_problem::d_scratch: what ccal_init_poses and validation() of every camera need (gathered values + the selection's work area)
inline size_t problem_scratch_hint(const ccal_problem* p) {
    return (size_t)std::max<int64_t>(p->n_corners, 1) * 32 + (size_t)(std::max(p->n_obs, 1) + 1) * 64 + (size_t)384 * 1024;
}
// the scratch holds at least pl.total bytes; a new block gets the test hook's poison over the plan's slices of doubles
hipError_t ensure_scratch(ccal_problem* p, const CallPlan& pl);
hipError_t validation_stats_device(ccal_problem* p, int cam, const double* d_err, double* avg_99, double* median, hipStream_t s);
hipError_t camera_errors_device(ccal_problem* p, int cam, const double* d_err, double** d_out, int64_t* n_out, hipStream_t s);     // *d_out: a slice of p->d_scratch
inline size_t order_stats_block_bytes(int64_t n, hipStream_t = nullptr) { return n <= 0 ? 0 : StatsScratch(0, n).plan.total; }     // block size order_stats_block needs for n values
hipError_t order_stats_block(char* block /* values in front */, size_t block_bytes, int64_t n, double* avg_99, double* median, hipStream_t s);
// ccal_api.hip: reprojection errors of every corner (only_cam >= 0: of that camera's) at the given parameters into p->d_err (device);
// ccal_multi.hip uses it per shard
int reprojection_errors_dev(ccal_problem* p, const double* intr, const double* poses, const double* extr, int only_cam = -1);
// ccal_kernels_init.hip
hipError_t launch_pose_init(const ccal_problem* p, int cam, const double* d_intr, double* d_poses_obs, int32_t* d_valid,
                            int min_points, hipStream_t s);
hipError_t launch_pose_init_division(const ccal_problem* p, int cam, double lambda, double* d_poses_obs, int32_t* d_valid,
                                     int min_points, hipStream_t s);
// ccal_kernels_pnp.hip: the general PnP for the frames with a corner off the z = 0 plane (the others are passed over), and for
// n_prob problems given as points + normalised image points (ccal_pnp_batch; d_cost may be nullptr)
hipError_t launch_pose_pnp(const ccal_problem* p, int cam, const double* d_intr, double* d_poses_obs, int32_t* d_valid,
                           int min_points, hipStream_t s);
hipError_t launch_pose_pnp_division(const ccal_problem* p, int cam, double lambda, double* d_poses_obs, int32_t* d_valid,
                                    int min_points, hipStream_t s);
hipError_t launch_pnp_batch(int n_prob, const int64_t* d_off, const double* d_xyz, const double* d_xn, int min_points,
                            double* d_poses, int32_t* d_n_used, double* d_cost, hipStream_t s);
// Dynamic LDS above 48 KiB has to be enabled per kernel AND per device: remember the largest size enabled on each
// device of this process (contexts on several GPUs may share the process).  Launchers run on any host thread
// (ccal_solve_batch / ccal_solve_sharded drive one thread per context): the fast path is one atomic load, the
// check-and-set runs under one process-wide mutex, so the attribute only ever grows and `enabled` never claims more
// than what was last set.
struct DynLdsGuard { std::atomic<size_t> enabled[16] = {}; };
inline std::mutex& dyn_lds_mutex() { static std::mutex m; return m; }
inline hipError_t ensure_dyn_lds(const void* fn, size_t lds, DynLdsGuard& g) {
    if (lds <= 48 * 1024) return hipSuccess;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::atomic<size_t>& have = g.enabled[dev & 15];
    if (lds <= have.load(std::memory_order_acquire)) return hipSuccess;
    std::lock_guard<std::mutex> lk(dyn_lds_mutex());
    if (lds <= have.load(std::memory_order_relaxed)) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) have.store(lds, std::memory_order_release);
    else (void)hipGetLastError();      // reported here: the runtime's sticky copy must not surface in an unrelated launcher's hipGetLastError()
    return e;
}

// ccal_multi.hip: the in-process transport of single-process sharded solves (shards on one GPU, or on GPUs with peer
// access when RCCL is not there) - events order the ranks' streams, the deciding kernel (k_head / k_solve) adds the ranks'
// buffers in rank order itself: PeerView = every rank's buffer of the step's sums, in its argument block.
constexpr int kMaxPeers = CCAL_MULTI_MAX_DEVICES;
struct PeerView { const double* src[kMaxPeers]; int32_t n; };
struct InprocComm;
InprocComm* inproc_create(int n, const int* devices, std::string* err);
void inproc_destroy(InprocComm* c);
void inproc_abort(InprocComm* c);                       // a rank failed: release the ranks waiting in the host rendezvous
bool inproc_aborted(const InprocComm* c);
int inproc_recover(InprocComm* c);                      // after an abort, no rank inside: drain the devices, reset the rendezvous
void inproc_set_timeout(InprocComm* c, double seconds); // host rendezvous: how long a rank waits for its peers (<= 0: 600 s)
void* inproc_rank_handle(InprocComm* c, int rank);      // ccal_problem::peer of that rank
int inproc_parity(const void* rank_handle);             // which of its two sum buffers the rank's next collective uses
int inproc_post(void* rank_handle, const double* device_buf, size_t count, void* hip_stream, PeerView* out);   // 0 = ok
// a context's persistent helper thread (ccal_solver_many.hip; created on first use): run fn on it / wait until it has finished
void ctx_worker_submit(ccal_ctx* ctx, std::function<void()> fn);
void ctx_worker_wait(ccal_ctx* ctx);
// One call over several contexts: fn(i) for i = 1 .. n - 1 on ctx[i]'s helper thread, `here` - fn(0) unless the caller has another body
// for its own thread - on the calling one; back when all have finished.  If a helper cannot be made (std::thread throws), `on_failure`
// runs - the sharded solve releases the ranks already started from their rendezvous with the one that will never come - what was
// handed out finishes, and the exception goes on to the caller.  fn must not throw.
template <class Fn, class Here, class OnFailure>
void ctx_fan_out(ccal_ctx* const* ctx, int n, Fn&& fn, Here&& here, OnFailure&& on_failure) {
    int started = 0;
    try { for (int i = 1; i < n; ++i) { ctx_worker_submit(ctx[i], [&fn, i] { fn(i); }); started = i; } }
    catch (...) { on_failure(); for (int i = 1; i <= started; ++i) ctx_worker_wait(ctx[i]); throw; }
    here();
    for (int i = 1; i < n; ++i) ctx_worker_wait(ctx[i]);
}
template <class Fn>
void ctx_fan_out(ccal_ctx* const* ctx, int n, Fn&& fn) { ctx_fan_out(ctx, n, fn, [&fn] { fn(0); }, [] {}); }
// a spinning host thread's pause between two looks
__attribute__((visibility("hidden"))) inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield" ::: "memory");
#else
    std::this_thread::yield();
#endif
}
// fn() -> ccal_status on a thread no exception may leave: its code, or the exception's, with the reason in the context (ctx may be NULL)
template <class Fn>
int guarded(ccal_ctx* ctx, const char* where, Fn&& fn) noexcept {
    try { return fn(); }
    catch (const std::bad_alloc&) { note_error(ctx, "out of host memory"); return CCAL_ERR_NO_MEMORY; }
    catch (...) { note_error(ctx, where); return CCAL_ERR_HIP; }
}
// the report of a call that ended without the solver's verdict
__attribute__((visibility("hidden"))) inline void blank_report(ccal_report* rep, int rc) { if (rep) { *rep = ccal_report{}; rep->status = rc; } }
// why the last ccal_ctx_create / ccal_multi_create* on this thread failed (ccal_create_last_error)
void note_create_error(const std::string& msg) noexcept;
// ccal_rccl.hip: communicators of one process, one per device (ncclCommInitAll); abort = ncclCommAbort
int rccl_comm_init_all(const int* devices, int n, void** comms_out, std::string* err);
void rccl_comm_abort(void* comm);
// ccal_solver_many.hip: n shards of ONE problem (distinct contexts, a transport set on every shard), each driven by a host
// thread of its own; `inproc` (may be NULL) is aborted when a rank fails
int solve_sharded_run(ccal_problem** shards, int n, const ccal_solver_opts* o, double* intr_io, double* const* poses_io,
                      double* extr_io, ccal_report* rep, InprocComm* inproc);

// ---- from pixels to detections: the four stages on device buffers --------------------------------------------------------------------
// Each stage's argument block, its parameter check (the message of the first range missed, or nullptr) and its launch sequence live
// in the stage's own translation unit, which keeps its compiler flags; the stage's entry points and ccal_detect_tags_*
// (ccal_kernels_tagchain.hip) enqueue through the same routines.  A routine only enqueues on `s` and returns hipGetLastError().
// Where DetectArgs and a chain's CornerArgs are filled, and the front both chains run per chunk (images to refined candidates):
// ccal_chain_front.hpp, host only.
// ccal_kernels_detect.hip
struct DetectArgs {
    const void* img;                    // [n][H][W] of T
    int32_t W, H, n;                    // n: images of this chunk
    int32_t s, r, rel_q10, cap;
    int64_t min_response;
    int32_t d0, dw, dh;                 // the domain: x in [d0, d0 + dw), y in [d0, d0 + dh)
    int32_t nbx, nby;                   // its (r+1) x (r+1) blocks
    int32_t* pix;                       // [n][nby * nbx]: y * W + x of the block's local maximum, -1: none
    int32_t* hess;                      // [n][nby * nbx][3]
    int64_t* resp;                      // [n][nby * nbx]
    long long* rmax;                    // [n]: max(0, the largest R of the domain)
    int32_t* rowoff;                    // [n][dh]: candidates of the image in front of the row
    int32_t* count;                     // [n]
    const int64_t* imgoff;              // [n + 1]: stored rows in front of the image
    int32_t* oxy; int32_t* ohess; int64_t* oresp;       // the stored rows of the chunk, image after image
};
const char* detect_bad_params(int step, int nms_radius, int64_t min_response, int rel_q10, int cap);
hipError_t detect_enqueue_find(hipStream_t s, int dtype, const DetectArgs& a);     // clears pix and rmax; tiles, rows: count[] is final
hipError_t detect_enqueue_emit(hipStream_t s, const DetectArgs& a);               // the stored rows, once imgoff[] is there
// ccal_kernels_corners.hip
struct CornerArgs {
    const void* img;                    // [n_img][H][W] of T
    const int64_t* off;                 // [n_img + 1]
    double* xy;                         // [n][2] in: start, out: result
    int32_t* status; int32_t* iters;    // [n]
    double* lam;                        // [n]
    int64_t n;                          // corners in all
    int32_t W, H, n_img;
    int32_t h, max_it;
    double eps;
};
const char* corners_bad_params(int half_win, int max_iterations, double eps);
hipError_t corners_enqueue(hipStream_t s, int dtype, const CornerArgs& a);
// ccal_kernels_quads.hip
struct QuadArgs {
    const void* img;                    // [n_img][H][W] of T, the chunk's first image first
    const int64_t* off;                 // [n_img + 1]: the caller's offsets of the chunk's images (not rebased)
    const double* xy;                   // [n][2], the chunk's first point first
    int32_t* adj;                       // [n][CCAL_QUAD_MAX_OUT_EDGES]: out-edge lists, indices local to the image; slots past min(deg, 8) unwritten
    int32_t* deg;                       // [n] full out-degree
    int32_t* cnt;                       // [n] quads whose smallest corner is the point
    const int32_t* base;                // [n] the rank, within its image, of the point's first quad (an exclusive scan of cnt)
    const int64_t* rowoff;              // [n_img + 1] the first stored row of each image in oidx / oquads
    int32_t* oidx;                      // [rows][4]
    double* oquads;                     // [rows][4][2] or NULL
    int64_t p0;                         // the caller's index of the chunk's first point = off[0]
    int64_t n;                          // points in the chunk
    int32_t W, H, n_img, K, cap;
    double min2, max2, ratio2, offset, min_contrast;
};
constexpr int64_t kQuadMaxPoints = 32768;     // per image: the pair search is quadratic
const char* quads_bad_params(double min_side, double max_side, double max_side_ratio, double offset, int samples, double min_contrast, int cap);
void quads_set_params(QuadArgs& a, double min_side, double max_side, double max_side_ratio, double offset, int samples, double min_contrast, int cap);
hipError_t quads_enqueue_count(hipStream_t s, int dtype, const QuadArgs& a);       // edges, then the count walk: adj, deg, cnt
hipError_t quads_enqueue_write(hipStream_t s, const QuadArgs& a);                 // the stored rows, once base[] and rowoff[] are there
// ccal_kernels_tags.hip
struct TagArgs {
    const void* img;                    // [n_img][H][W] of T, the chunk's first image first
    const int64_t* off;                 // [n_img + 1]: the caller's offsets of the chunk's images (not rebased)
    const double* quads;                // [n][4][2], the chunk's first quad first
    const unsigned long long* codes;    // [n_codes]
    int32_t* reason; int32_t* id; int32_t* rot; int32_t* hamming;      // [n]
    double* corners;                    // [n][4][2]
    unsigned long long* code;           // [n]
    double* margin;                     // [n]
    int64_t q0;                         // the caller's index of the chunk's first quad = off[0]
    int64_t n;                          // quads in the chunk
    int32_t W, H, n_img;
    int32_t d, border, n_codes, S;
    int32_t max_border, max_hamming;
    double min_contrast;
};
const char* tags_bad_params(int d, int border, int n_codes, int samples, double min_contrast, int max_border_errors, int max_hamming);
const char* tags_bad_codes(int d, const uint64_t* codes, int n_codes);       // the table, once the ranges hold
hipError_t tags_enqueue(hipStream_t s, int dtype, const TagArgs& a);
// ccal_kernels_tagchain.hip: the two decision kernels of ccal_detect_tags_* on device arrays (the second library's test entry points
// run them alone, ccal_legacy_test_hooks.hip)
struct MergeArgs {
    const int64_t* off;                 // [n_img + 1]: image k owns the points [off[k], off[k + 1]) of xy, status and out
    const double* xy;                   // [.][2]
    const int32_t* status;              // [.] only CCAL_OK goes on; NULL: every point does
    double* out;                        // [.][2]: the kept points of image k from off[k] on, in order
    int32_t* kept;                      // [n_img]
    int32_t n_img, cap;                 // cap: the most points of one image (the walk's clamp)
    double radius;
};
hipError_t tagchain_enqueue_merge(hipStream_t s, const MergeArgs& a);
struct SelectArgs {
    const int64_t* off;                 // [n_img + 1]: image k owns the rows [off[k], off[k + 1]) of the decoder's outputs
    const int32_t* reason; const int32_t* id; const int32_t* rot; const int32_t* hamming;
    const double* corners; const double* margin;
    int32_t* win;                       // [.] work: 1 for the row that keeps its id
    int32_t* count; int32_t* n_ok;      // [n_img]: distinct ids, CCAL_TAG_OK rows
    int32_t* oid; int32_t* orot; int32_t* oham;         // [n_img][rows]
    double* ocorners; double* omargin;  // [n_img][rows][4][2], [n_img][rows]
    int32_t n_img, cap, rows;           // cap: the most quads of one image (the walk's clamp); rows: tags stored per image
};
hipError_t tagchain_enqueue_select(hipStream_t s, const SelectArgs& a);
// the chain's two plain links, which ccal_detect_checkerboards_* (ccal_kernels_board.hip) shares: off[k + 1] = the sum over i <= k of
// min(count[i], cap), off[0] = 0; and n stored int32 values as f64
hipError_t tagchain_enqueue_offsets(hipStream_t s, const int32_t* count, size_t cap, size_t n, int64_t* off);
hipError_t tagchain_enqueue_starts(hipStream_t s, const int32_t* in, double* out, int64_t n);
}  // namespace ccal

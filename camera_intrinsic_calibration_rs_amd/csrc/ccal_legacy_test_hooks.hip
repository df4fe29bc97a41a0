// Entry points of the SECOND library only (-DCCAL_TEST_HOOKS, libccal_hip_legacy.so): what the tests need to reach code that no
// call of include/ccal.h reaches with data of their choice.  Not declared in the header, not in _ffi.SYMBOLS; the product
// library does not contain this translation unit.
#include "ccal_call.hpp"
#include "ccal_device.hpp"
#include "ccal_fused.hpp"
#include "ccal_normal.hpp"
#include "ccal_pose_init.hpp"

// The radix select of validation() on raw values (tests/test_gpu_order_stats.py): vals[n] (host) -> the two statistics, through
// order_stats_block - the multi-GPU path's call, the product's kernels (build/ccal_kernels_stats.o is in both libraries).
extern "C" int ccal_test_order_stats(ccal_ctx* ctx, const double* vals, int64_t n, double* avg_99, double* median) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    if (!vals || n <= 0 || !avg_99 || !median) return ccal::fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_test_order_stats: n > 0 values and both outputs");
    CCAL_API_TRY
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t bytes = ccal::order_stats_block_bytes(n, ctx->stream);
    char* block = nullptr;
    hipError_t e = ccal::ctx_dev_alloc(ctx, (void**)&block, bytes);
    if (e != hipSuccess) return ccal::hip_fail(ctx, "ccal_test_order_stats: allocation", e);
    e = hipMemcpyAsync(block, vals, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = ccal::order_stats_block(block, bytes, n, avg_99, median, ctx->stream);
    (void)hipStreamSynchronize(ctx->stream);            // nothing in flight uses the block when it goes back to the context
    ccal::ctx_release(ctx, block, false);
    if (e != hipSuccess) return ccal::hip_fail(ctx, "ccal_test_order_stats", e);
    return CCAL_OK;
    CCAL_API_CATCH(ctx)
}

// The f64 device math of ccal_device.hpp on inputs of the tests' choice (tests/test_gpu_device_math.py): one element per lane,
// grid-stride, the header's functions as they are.  Flat doubles per element, in -> out:
//   0 RCP x -> y | 1 SQRT_RSQRT x -> s, rs | 2 SINCOS x -> s, c | 3 ATAN2_POS r, z -> theta | 4 SO3 w[3] -> R[9], J_l[9] |
//   5 HUBER_SW s, delta -> sw
namespace {
constexpr int kDmOps = 6;
constexpr int kDmIn[kDmOps] = { 1, 1, 1, 2, 3, 2 }, kDmOut[kDmOps] = { 1, 2, 2, 1, 18, 1 };

__global__ void __launch_bounds__(256) k_test_device_math(int op, int64_t n, const double* __restrict__ in, double* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        switch (op) {
        case 0: out[i] = ccal::fast_rcp(in[i]); break;
        case 1: { double s, rs; ccal::fast_sqrt_rsqrt(in[i], s, rs); out[2 * i] = s; out[2 * i + 1] = rs; } break;
        case 2: { double s, c; ccal::fast_sincos(in[i], s, c); out[2 * i] = s; out[2 * i + 1] = c; } break;
        case 3: out[i] = ccal::fast_atan2_pos(in[2 * i], in[2 * i + 1]); break;
        case 4: {
            const double w[3] = { in[3 * i], in[3 * i + 1], in[3 * i + 2] };
            double R[9], JL[9];
            ccal::so3_exp_ljac(w, R, JL);
#pragma unroll
            for (int j = 0; j < 9; ++j) { out[18 * i + j] = R[j]; out[18 * i + 9 + j] = JL[j]; }
        } break;
        default: out[i] = ccal::huber_sqrt_weight(in[2 * i], in[2 * i + 1]); break;
        }
    }
}
}  // namespace

extern "C" int ccal_test_device_math(ccal_ctx* ctx, int op, int64_t n, const double* in, double* out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    if (op < 0 || op >= kDmOps || n <= 0 || !in || !out)
        return ccal::fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_test_device_math: a known op, n > 0 elements and both arrays");
    CCAL_API_TRY
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t in_bytes = (size_t)n * kDmIn[op] * sizeof(double), out_bytes = (size_t)n * kDmOut[op] * sizeof(double);
    char* block = nullptr;
    hipError_t e = ccal::ctx_dev_alloc(ctx, (void**)&block, in_bytes + out_bytes);
    if (e != hipSuccess) return ccal::hip_fail(ctx, "ccal_test_device_math: allocation", e);
    double* d_in = (double*)block;
    double* d_out = (double*)(block + in_bytes);
    e = hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        const int64_t blocks = (n + 255) / 256;
        k_test_device_math<<<dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, ctx->stream>>>(op, n, d_in, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);        // nothing in flight uses the block when it goes back to the context
    ccal::ctx_release(ctx, block, false);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return ccal::hip_fail(ctx, "ccal_test_device_math", e);
    return CCAL_OK;
    CCAL_API_CATCH(ctx)
}

// The pose initialisation's model inverse on pixels of the tests' choice (tests/test_gpu_model_inverse.py): unproject_normalized of
// ccal_pose_init.hpp as it is, one row per lane, grid-stride, with the context's ModelRt.  model: a camera model of include/ccal.h
// with its params() vector, or 100 (kUnprojDivision) with th = [half, half, w/2, h/2, lambda].  uv [n][2] -> xn_yn_out [n][2]
// (NaN where there is no ray), valid_out [n].
namespace {
struct UnprojNormArgs { double th[CCAL_PMAX]; double small_radius; int64_t n; const double* uv; double* out; uint8_t* valid; };

template <int MODEL>
__global__ void __launch_bounds__(256) k_test_unproject_normalized(const UnprojNormArgs a) {
    const double nan = __builtin_nan("");
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        double xn = nan, yn = nan;
        const bool ok = ccal::unproject_normalized<MODEL>(a.th, a.small_radius, a.uv[2 * i], a.uv[2 * i + 1], xn, yn);
        a.out[2 * i] = ok ? xn : nan; a.out[2 * i + 1] = ok ? yn : nan;
        a.valid[i] = ok ? 1 : 0;
    }
}
template <int M> struct LaunchUnprojNorm {
    static void go(int g, hipStream_t st, const UnprojNormArgs& a) { k_test_unproject_normalized<M><<<dim3(g), dim3(256), 0, st>>>(a); }
};
}  // namespace

extern "C" int ccal_test_unproject_normalized(ccal_ctx* ctx, int model, const double* params, int64_t n, const double* uv,
                                              double* xn_yn_out, uint8_t* valid_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    const char* where = "ccal_test_unproject_normalized";
    if (!params || n <= 0 || !uv || !xn_yn_out || !valid_out)
        return ccal::fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_test_unproject_normalized: params, n > 0 pixels and both outputs");
    const bool division = model == ccal::kUnprojDivision;
    if (!division) { if (const int rc = ccal::check_model(ctx, model, where)) return rc; }
    CCAL_API_TRY
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    UnprojNormArgs a = {};
    if (division) { for (int i = 0; i < 5; ++i) a.th[i] = params[i]; a.small_radius = ccal::model_rt(ctx).unproject_eps; }
    else { ccal::ModelRt rt; ccal::canonical_theta(ctx, model, params, a.th, &rt); a.small_radius = rt.unproject_eps; }
    const size_t xy_bytes = (size_t)n * 2 * sizeof(double);
    char* block = nullptr;
    hipError_t e = ccal::ctx_dev_alloc(ctx, (void**)&block, 2 * xy_bytes + (size_t)n);
    if (e != hipSuccess) return ccal::hip_fail(ctx, "ccal_test_unproject_normalized: allocation", e);
    a.n = n; a.uv = (const double*)block; a.out = (double*)(block + xy_bytes); a.valid = (uint8_t*)(block + 2 * xy_bytes);
    e = hipMemcpyAsync(block, uv, xy_bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        const int64_t blocks = (n + 255) / 256;
        const int g = (int)(blocks < 1024 ? blocks : 1024);
        if (division) LaunchUnprojNorm<ccal::kUnprojDivision>::go(g, ctx->stream, a);
        else ccal::launch_model<LaunchUnprojNorm>(model, g, ctx->stream, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(xn_yn_out, a.out, xy_bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(valid_out, a.valid, (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);        // nothing in flight uses the block when it goes back to the context
    ccal::ctx_release(ctx, block, false);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return ccal::hip_fail(ctx, where, e);
    return CCAL_OK;
    CCAL_API_CATCH(ctx)
}

// The two decision kernels of ccal_detect_tags_* alone, on arrays of the tests' choice (tests/test_gpu_detect_tags.py).  The output
// arrays go to the device as the caller filled them and come back whole: what a kernel does not write keeps the caller's value.
namespace {
int hook_offsets(ccal_ctx* ctx, const char* where, int n_img, const int64_t* offsets, size_t* most) {
    if (n_img < 1 || !offsets) return ccal::fail(ctx, CCAL_ERR_INVALID_ARG, "a test hook: n_img >= 1 and offsets");
    if (ccal::check_offsets(ctx, where, "offsets", offsets, (size_t)n_img, 0)) return CCAL_ERR_INVALID_ARG;
    if (offsets[n_img] > (int64_t)INT32_MAX) return ccal::fail(ctx, CCAL_ERR_INVALID_ARG, "a test hook: more than 2^31 - 1 rows");
    *most = 0;
    for (int k = 0; k < n_img; ++k) *most = std::max(*most, (size_t)(offsets[k + 1] - offsets[k]));
    return CCAL_OK;
}
}  // namespace

// image k owns the points [offsets[k], offsets[k + 1]); status NULL: every point goes on.  kept_out [n_img]; xy_out [.][2]: the kept
// points of image k from offsets[k] on
extern "C" int ccal_test_merge_points(ccal_ctx* ctx, int n_img, const int64_t* offsets, const double* xy, const int32_t* status,
                                      double radius, int32_t* kept_out, double* xy_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    const char* where = "ccal_test_merge_points";
    size_t most = 0;
    if (const int rc = hook_offsets(ctx, where, n_img, offsets, &most)) return rc;
    if (!kept_out || !(radius >= 0.0)) return ccal::fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_test_merge_points: kept_out and a radius >= 0");
    const size_t n = (size_t)offsets[n_img], ni = (size_t)n_img;
    if (n && (!xy || !xy_out)) return ccal::fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_test_merge_points: both point arrays");
    ccal::CallBlock blk(ctx);
    const auto s_off = blk.add<int64_t>(ni + 1);
    const auto s_status = blk.add<int32_t>(status ? n : 0);
    const auto s_kept = blk.add<int32_t>(ni);
    const auto s_xy = blk.add<double>(2 * n);
    const auto s_out = blk.add<double>(2 * n);
    if (!blk.alloc()) return blk.finish(where);
    blk.upload(s_off, offsets, ni + 1);
    if (status) blk.upload(s_status, status, n);
    blk.upload(s_xy, xy, 2 * n);
    blk.upload(s_out, xy_out, 2 * n);
    ccal::MergeArgs a = {};
    a.off = blk.at(s_off); a.xy = blk.at(s_xy); a.status = blk.at(s_status); a.out = blk.at(s_out); a.kept = blk.at(s_kept);
    a.n_img = n_img; a.cap = (int32_t)most; a.radius = radius;
    if (blk.ok()) blk.note(ccal::tagchain_enqueue_merge(ctx->stream, a));
    blk.download(kept_out, a.kept, ni);
    blk.download(xy_out, a.out, 2 * n);
    return blk.finish(where);
    CCAL_API_CATCH(ctx)
}

// image k owns the decoder's rows [offsets[k], offsets[k + 1]); outputs [n_img] and [n_img][rows]
extern "C" int ccal_test_select_tags(ccal_ctx* ctx, int n_img, const int64_t* offsets, const int32_t* reason, const int32_t* id,
                                     const int32_t* rot, const int32_t* hamming, const double* corners, const double* margin, int rows,
                                     int32_t* count_out, int32_t* n_ok_out, int32_t* id_out, int32_t* rot_out, int32_t* hamming_out,
                                     double* corners_out, double* margin_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    const char* where = "ccal_test_select_tags";
    size_t most = 0;
    if (const int rc = hook_offsets(ctx, where, n_img, offsets, &most)) return rc;
    const size_t n = (size_t)offsets[n_img], ni = (size_t)n_img;
    if (rows < 1 || !count_out || !n_ok_out || !id_out || !rot_out || !hamming_out || !corners_out || !margin_out ||
        (n && (!reason || !id || !rot || !hamming || !corners || !margin)))
        return ccal::fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_test_select_tags: rows >= 1 and every array");
    const size_t t = (size_t)rows * ni;
    ccal::CallBlock blk(ctx);
    const auto s_off = blk.add<int64_t>(ni + 1);
    const auto s_reason = blk.add<int32_t>(n);
    const auto s_id = blk.add<int32_t>(n);
    const auto s_rot = blk.add<int32_t>(n);
    const auto s_ham = blk.add<int32_t>(n);
    const auto s_win = blk.add<int32_t>(n);
    const auto s_count = blk.add<int32_t>(ni);
    const auto s_nok = blk.add<int32_t>(ni);
    const auto s_oid = blk.add<int32_t>(t);
    const auto s_orot = blk.add<int32_t>(t);
    const auto s_oham = blk.add<int32_t>(t);
    const auto s_corners = blk.add<double>(8 * n);
    const auto s_margin = blk.add<double>(n);
    const auto s_ocorners = blk.add<double>(8 * t);
    const auto s_omargin = blk.add<double>(t);
    if (!blk.alloc()) return blk.finish(where);
    blk.upload(s_off, offsets, ni + 1);
    blk.upload(s_reason, reason, n); blk.upload(s_id, id, n); blk.upload(s_rot, rot, n); blk.upload(s_ham, hamming, n);
    blk.upload(s_corners, corners, 8 * n); blk.upload(s_margin, margin, n);
    blk.upload(s_oid, id_out, t); blk.upload(s_orot, rot_out, t); blk.upload(s_oham, hamming_out, t);
    blk.upload(s_ocorners, corners_out, 8 * t); blk.upload(s_omargin, margin_out, t);
    ccal::SelectArgs a = {};
    a.off = blk.at(s_off); a.reason = blk.at(s_reason); a.id = blk.at(s_id); a.rot = blk.at(s_rot); a.hamming = blk.at(s_ham);
    a.corners = blk.at(s_corners); a.margin = blk.at(s_margin); a.win = blk.at(s_win); a.count = blk.at(s_count); a.n_ok = blk.at(s_nok);
    a.oid = blk.at(s_oid); a.orot = blk.at(s_orot); a.oham = blk.at(s_oham); a.ocorners = blk.at(s_ocorners); a.omargin = blk.at(s_omargin);
    a.n_img = n_img; a.cap = (int32_t)most; a.rows = rows;
    if (blk.ok()) blk.note(ccal::tagchain_enqueue_select(ctx->stream, a));
    blk.download(count_out, a.count, ni);
    blk.download(n_ok_out, a.n_ok, ni);
    blk.download(id_out, a.oid, t); blk.download(rot_out, a.orot, t); blk.download(hamming_out, a.oham, t);
    blk.download(corners_out, a.ocorners, 8 * t); blk.download(margin_out, a.omargin, t);
    return blk.finish(where);
    CCAL_API_CATCH(ctx)
}

// The proof that CallBlock's guard mode (CCAL_TEST_GUARD_SLICES, ccal_call.hpp) sees a stray write (tests/test_gpu_guard.py): a block
// of three slices - double x 5, an absent one, int32_t x 65 - of which the host damages ONE byte, `delta` bytes from the exact end
// (from_end != 0) or from the start of slice 0 or 2, with a memset on the context's stream; the status is finish()'s.  A position
// outside the block's own allocation (the byte in front of slice 0 without the guard mode) is not written.
extern "C" int ccal_test_guard_damage(ccal_ctx* ctx, int slice, int from_end, int64_t delta) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    const char* where = "ccal_test_guard_damage";
    if (slice != 0 && slice != 2) return ccal::fail(ctx, CCAL_ERR_INVALID_ARG, "ccal_test_guard_damage: slice 0 or 2");
    ccal::CallBlock blk(ctx);
    const auto s_a = blk.add<double>(5);
    const auto s_none = blk.add<double>(0);
    const auto s_c = blk.add<int32_t>(65);
    (void)s_none;
    if (!blk.alloc()) return blk.finish(where);
    blk.memset(s_a, 0, 5);
    blk.memset(s_c, 0, 65);
    const int64_t pos = (int64_t)(slice == 0 ? s_a.off : s_c.off) + (from_end ? (slice == 0 ? 5 * (int64_t)sizeof(double) : 65 * (int64_t)sizeof(int32_t)) : 0) + delta;
    if (pos >= 0 && pos < (int64_t)blk.total && blk.ok())
        blk.note(hipMemsetAsync(reinterpret_cast<char*>(blk.at(s_a)) - s_a.off + pos, 0x3C, 1, ctx->stream));
    return blk.finish(where);
    CCAL_API_CATCH(ctx)
}

// The two small dense solves at the end of every step, on systems of the tests' choice (tests/test_gpu_camera_solve.py): k_solve
// (launch_solve's geometry: test_launch_solve, ccal_kernels_normal.hip) or k_head (launch_head), and k_backsub (test_launch_backsub) -
// the kernels as they are, device-resident form, on a state as launch_state_eval leaves it (first evaluation, method from lambda) with
// set `cur` as the current one.  Every in / out array is [guard | payload | guard] doubles, goes to the device as the caller filled
// it and comes back whole: what a kernel does not write keeps the caller's value, the kernels get the payload's address.
//   form 0 k_solve: red [red_size(K)], 1 <= K < CCAL_KMAX;  form 1 k_head: red [fused_red_size(K)], 4 <= K <= 9, n_intr = CCAL_PMAX, n_extr = 0
//   cols [K] of col_bytes = sizeof(ColInfo) each;  intr0/1 [n_intr + tail], extr0/1 [n_extr + tail], dc [CCAL_KMAX]: payloads
//   state_out [8]: mc_cam, lambda_solve, done, cam_failed, cur, first, flags[1], scal[2] (k_head: the last two stay as they came)
namespace {
struct HookBlock {          // one block of the context's allocator cut into 256-byte aligned pieces; a sticky status like CallBlock's
    ccal_ctx* ctx; char* base = nullptr; size_t total = 0; hipError_t e = hipSuccess;
    explicit HookBlock(ccal_ctx* c) : ctx(c) {}
    ~HookBlock() { if (base) { (void)hipStreamSynchronize(ctx->stream); ccal::ctx_release(ctx, base, false); } }
    size_t add(size_t bytes) { const size_t off = total; total += (bytes + 255) & ~(size_t)255; return off; }
    bool alloc() { e = hipSetDevice(ctx->device); if (e == hipSuccess) e = ccal::ctx_dev_alloc(ctx, (void**)&base, total); return e == hipSuccess; }
    template <class T> T* at(size_t off) const { return reinterpret_cast<T*>(base + off); }
    void note(hipError_t r) { if (e == hipSuccess) e = r; }
    void up(size_t off, const void* host, size_t bytes) { if (e == hipSuccess && bytes) e = hipMemcpyAsync(base + off, host, bytes, hipMemcpyHostToDevice, ctx->stream); }
    void down(void* host, size_t off, size_t bytes) { if (e == hipSuccess && bytes) e = hipMemcpyAsync(host, base + off, bytes, hipMemcpyDeviceToHost, ctx->stream); }
    void zero(size_t off, size_t bytes) { if (e == hipSuccess) e = hipMemsetAsync(base + off, 0, bytes, ctx->stream); }
    int finish(const char* where) {
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        return e == hipSuccess ? CCAL_OK : ccal::hip_fail(ctx, where, e);
    }
};
ccal::DevState hook_state(double lambda, int cur) {
    ccal::DevState st = {};
    st.lambda = lambda; st.lambda_spec = lambda; st.lambda_solve = -1.0;        // (k_state_eval: 0; -1 shows the kernel's store in Gauss-Newton too)
    st.radius = lambda > 0.0 ? 1.0 / lambda : 1e4; st.dec = 2.0;
    st.mc_cam = __builtin_nan("");
    st.min_error = 1e-10; st.min_abs = 1e-5; st.min_rel = 1e-5;
    st.cur = cur; st.first = 1; st.max_iter = 100;
    st.method = lambda > 0.0 ? CCAL_METHOD_LM : CCAL_METHOD_GN;
    return st;
}
constexpr int kHookMaxGuard = 4096, kHookMaxParams = 1024, kHookMaxSlots = 4096;
}  // namespace

extern "C" int ccal_test_camera_solve(ccal_ctx* ctx, int form, int K, const double* red, const void* cols, int col_bytes, int n_intr, int n_extr,
                                      int guard, int tail, double* intr0, double* intr1, double* extr0, double* extr1,
                                      double lambda, double min_diag, double max_diag, int cur, double* dc, double* state_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    const char* where = "ccal_test_camera_solve";
    const ccal::BadArg bad{ ctx, where };
    if (form != 0 && form != 1) return bad("form 0 (k_solve) or 1 (k_head)");
    if (form == 0 ? (K < 1 || K >= CCAL_KMAX) : (K < 4 || K > ccal::kFusedMaxK)) return bad("K outside the form's sizes");
    if (col_bytes != (int)sizeof(ccal::ColInfo)) return bad("col_bytes is not the size of a column record");
    if (guard < 0 || guard > kHookMaxGuard || tail < 0 || tail > kHookMaxGuard) return bad("guard and tail: 0 .. 4096 doubles");
    if (form == 0 ? (n_intr < 1 || n_intr > kHookMaxParams) : n_intr != CCAL_PMAX) return bad("n_intr outside the form's sizes");
    if (form == 0 ? (n_extr < 0 || n_extr > kHookMaxParams) : n_extr != 0) return bad("n_extr outside the form's sizes");
    if (cur != 0 && cur != 1) return bad("cur 0 or 1");
    if (!(lambda >= 0.0) || !(lambda < 1.7e308)) return bad("lambda: finite, >= 0");
    if (!(min_diag <= max_diag)) return bad("min_diag <= max_diag");
    if (!red || !cols || !intr0 || !intr1 || !extr0 || !extr1 || !dc || !state_out) return bad("every array");
    const ccal::ColInfo* ci = static_cast<const ccal::ColInfo*>(cols);
    for (int i = 0; i < K; ++i) {
        const int n = ci[i].is_extr ? n_extr : n_intr;
        if (ci[i].is_extr != 0 && ci[i].is_extr != 1) return bad("a column's is_extr is 0 or 1");
        if (ci[i].dst < 0 || ci[i].dst >= n) return bad("a column's dst outside its parameter array");
        if (ci[i].dst2 < -1 || ci[i].dst2 >= n) return bad("a column's dst2 outside its parameter array");
    }
    const size_t g = (size_t)guard, D = sizeof(double);
    const size_t n_red = (size_t)(form == 0 ? ccal::red_size(K) : ccal::fused_red_size(K));
    const size_t len_i = 2 * g + (size_t)n_intr + (size_t)tail, len_e = 2 * g + (size_t)n_extr + (size_t)tail, len_dc = 2 * g + CCAL_KMAX;
    HookBlock blk(ctx);
    const size_t o_red = blk.add(n_red * D), o_cols = blk.add((size_t)K * sizeof(ccal::ColInfo));
    const size_t o_i0 = blk.add(len_i * D), o_i1 = blk.add(len_i * D), o_e0 = blk.add(len_e * D), o_e1 = blk.add(len_e * D);
    const size_t o_dc = blk.add(len_dc * D), o_scal = blk.add(8 * D), o_flags = blk.add(4 * sizeof(int32_t));
    const size_t o_st = blk.add(sizeof(ccal::DevState)), o_hs = blk.add(sizeof(ccal::HostStatus));
    if (!blk.alloc()) return blk.finish(where);
    const ccal::DevState st0 = hook_state(lambda, cur);
    blk.up(o_red, red, n_red * D); blk.up(o_cols, cols, (size_t)K * sizeof(ccal::ColInfo));
    blk.up(o_i0, intr0, len_i * D); blk.up(o_i1, intr1, len_i * D); blk.up(o_e0, extr0, len_e * D); blk.up(o_e1, extr1, len_e * D);
    blk.up(o_dc, dc, len_dc * D); blk.up(o_st, &st0, sizeof st0);
    blk.zero(o_scal, 8 * D); blk.zero(o_flags, 4 * sizeof(int32_t)); blk.zero(o_hs, sizeof(ccal::HostStatus));
    if (blk.e == hipSuccess) {
        if (form == 0) {
            ccal::TestSolveIO t = {};
            t.red = blk.at<double>(o_red); t.cols = blk.at<ccal::ColInfo>(o_cols); t.K = K; t.min_diag = min_diag; t.max_diag = max_diag;
            t.intr[0] = blk.at<double>(o_i0) + g; t.intr[1] = blk.at<double>(o_i1) + g;
            t.extr[0] = blk.at<double>(o_e0) + g; t.extr[1] = blk.at<double>(o_e1) + g;
            t.n_intr = n_intr; t.n_extr = n_extr;
            t.dc = blk.at<double>(o_dc) + g; t.scal = blk.at<double>(o_scal); t.flags = blk.at<int32_t>(o_flags);
            t.st = blk.at<ccal::DevState>(o_st); t.hs = blk.at<ccal::HostStatus>(o_hs);
            blk.note(ccal::test_launch_solve(t, ctx->stream));
        } else {
            ccal::HeadArgs a = {};
            a.st = blk.at<ccal::DevState>(o_st); a.hs = blk.at<ccal::HostStatus>(o_hs); a.red = blk.at<double>(o_red);
            a.cols = blk.at<ccal::ColInfo>(o_cols);
            a.intr[0] = blk.at<double>(o_i0) + g; a.intr[1] = blk.at<double>(o_i1) + g; a.dc = blk.at<double>(o_dc) + g;
            a.K = K; a.seq = 1; a.min_diag = min_diag; a.max_diag = max_diag;
            blk.note(ccal::launch_head(a, ctx->stream));
        }
    }
    ccal::DevState st1 = {};
    double scal[8] = {}; int32_t flags[4] = {};
    blk.down(intr0, o_i0, len_i * D); blk.down(intr1, o_i1, len_i * D); blk.down(extr0, o_e0, len_e * D); blk.down(extr1, o_e1, len_e * D);
    blk.down(dc, o_dc, len_dc * D); blk.down(&st1, o_st, sizeof st1); blk.down(scal, o_scal, sizeof scal); blk.down(flags, o_flags, sizeof flags);
    if (const int rc = blk.finish(where)) return rc;
    state_out[0] = st1.mc_cam; state_out[1] = st1.lambda_solve; state_out[2] = st1.done; state_out[3] = st1.cam_failed;
    state_out[4] = st1.cur; state_out[5] = st1.first;
    if (form == 0) { state_out[6] = flags[1]; state_out[7] = scal[2]; }
    return CCAL_OK;
    CCAL_API_CATCH(ctx)
}

// k_backsub on records of the tests' choice: pf [n_slots][pf_size(K)], dc_in [K]; poses0 / poses1 [guard | n_slots * 6 | guard] (set
// `cur` is read, the other one written), mc_slot [guard | n_slots | guard]: in / out, whole, as above.
extern "C" int ccal_test_backsub(ccal_ctx* ctx, int n_slots, int K, const double* pf, const double* dc_in, int guard,
                                 double* poses0, double* poses1, double lambda, double min_diag, double max_diag, int cur, double* mc_slot) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    const char* where = "ccal_test_backsub";
    const ccal::BadArg bad{ ctx, where };
    if (n_slots < 1 || n_slots > kHookMaxSlots) return bad("n_slots: 1 .. 4096");
    if (K < 1 || K >= CCAL_KMAX) return bad("K: 1 .. CCAL_KMAX - 1");
    if (guard < 0 || guard > kHookMaxGuard) return bad("guard: 0 .. 4096 doubles");
    if (cur != 0 && cur != 1) return bad("cur 0 or 1");
    if (!(lambda >= 0.0) || !(lambda < 1.7e308)) return bad("lambda: finite, >= 0");
    if (!(min_diag <= max_diag)) return bad("min_diag <= max_diag");
    if (!pf || !dc_in || !poses0 || !poses1 || !mc_slot) return bad("every array");
    const size_t g = (size_t)guard, D = sizeof(double), ns = (size_t)n_slots, PF = (size_t)ccal::pf_size(K);
    const size_t len_p = 2 * g + 6 * ns, len_m = 2 * g + ns;
    HookBlock blk(ctx);
    const size_t o_pf = blk.add(ns * PF * D), o_dc = blk.add((size_t)K * D), o_p0 = blk.add(len_p * D), o_p1 = blk.add(len_p * D);
    const size_t o_mc = blk.add(len_m * D), o_st = blk.add(sizeof(ccal::DevState));
    if (!blk.alloc()) return blk.finish(where);
    ccal::DevState st0 = hook_state(lambda, cur);
    st0.first = 0;                                    // behind a k_solve that has decided and solved
    blk.up(o_pf, pf, ns * PF * D); blk.up(o_dc, dc_in, (size_t)K * D); blk.up(o_p0, poses0, len_p * D); blk.up(o_p1, poses1, len_p * D);
    blk.up(o_mc, mc_slot, len_m * D); blk.up(o_st, &st0, sizeof st0);
    if (blk.e == hipSuccess) {
        ccal::TestBacksubIO t = {};
        t.pf = blk.at<double>(o_pf); t.dc = blk.at<double>(o_dc); t.mc_slot = blk.at<double>(o_mc) + g;
        t.poses[0] = blk.at<double>(o_p0) + g; t.poses[1] = blk.at<double>(o_p1) + g;
        t.n_slots = n_slots; t.K = K; t.min_diag = min_diag; t.max_diag = max_diag; t.st = blk.at<ccal::DevState>(o_st);
        blk.note(ccal::test_launch_backsub(t, ctx->stream));
    }
    blk.down(poses0, o_p0, len_p * D); blk.down(poses1, o_p1, len_p * D); blk.down(mc_slot, o_mc, len_m * D);
    return blk.finish(where);
    CCAL_API_CATCH(ctx)
}

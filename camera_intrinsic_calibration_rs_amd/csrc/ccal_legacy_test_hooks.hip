// Entry points of the SECOND library only (-DCCAL_TEST_HOOKS, libccal_hip_legacy.so): what the tests need to reach code that no
// call of include/ccal.h reaches with data of their choice.  Not declared in the header, not in _ffi.SYMBOLS; the product
// library does not contain this translation unit.
#include "ccal_call.hpp"
#include "ccal_device.hpp"
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

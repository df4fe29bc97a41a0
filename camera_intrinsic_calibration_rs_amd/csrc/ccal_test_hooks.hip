// Entry points of the SECOND library only (-DCCAL_TEST_HOOKS, libccal_hip_legacy.so): what the tests need to reach code that no
// call of include/ccal.h reaches with data of their choice.  Not declared in the header, not in _ffi.SYMBOLS; the product
// library links this translation unit as an empty object.
#ifdef CCAL_TEST_HOOKS
#include "ccal_call.hpp"
#include "ccal_device.hpp"

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
#endif

// Entry points of the SECOND library only (-DCCAL_TEST_HOOKS, libccal_hip_legacy.so): what the tests need to reach code that no
// call of include/ccal.h reaches with data of their choice.  Not declared in the header, not in _ffi.SYMBOLS; the product
// library links this translation unit as an empty object.
#ifdef CCAL_TEST_HOOKS
#include "ccal_call.hpp"

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
#endif

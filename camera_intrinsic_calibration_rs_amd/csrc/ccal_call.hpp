// One-shot batch calls (host arrays in, host arrays out): ONE device block of the context's allocator, cut into slices that each
// start on a 256-byte boundary; uploads, the launch, downloads and one synchronise, all on the context's stream.
//   CallPlan   the slices in order and the total - plain arithmetic, no context and no HIP call (ccal_plan.hpp)
//   CallBlock  the plan, the block and a sticky hipError_t: after the first failure every step is a no-op and finish() reports it;
//              the destructor drains the stream before the block goes back to the context's cache, on every way out
//   check_offsets  the argument check of a batched call's CSR offsets, with the call's name in the message
// Host only; for the translation units of the one-shot entry points ("One-shot calls").
#pragma once
#include <cstdio>
#include "ccal_internal.hpp"
#include "ccal_plan.hpp"

namespace ccal {

// the two ways out of a one-shot entry point with the context's message set: a status of the caller's choice / CCAL_ERR_HIP "<where>: <HIP's text>"
inline int fail(ccal_ctx* ctx, int code, const char* msg) { note_error(ctx, msg); return code; }
inline int hip_fail(ccal_ctx* ctx, const char* where, hipError_t e) {
    try { ctx->err = std::string(where) + ": " + hipGetErrorString(e); } catch (...) { }
    return CCAL_ERR_HIP;
}

// offsets[0] == 0, then over the n problems offsets[0 .. n]: no decrease and, with max_span > 0 (2^24, what the kernels index a
// problem by), no problem of more points.  CCAL_OK, or CCAL_ERR_INVALID_ARG with "<where>: <name>..." as the context's message.
inline int check_offsets(ccal_ctx* ctx, const char* where, const char* name, const int64_t* offsets, size_t n, int64_t max_span) {
    const char* bad = offsets[0] != 0 ? "%s: %s[0] != 0" : nullptr;
    for (size_t i = 0; i < n && !bad; ++i)
        if (offsets[i + 1] < offsets[i] || (max_span > 0 && offsets[i + 1] - offsets[i] > max_span))
            bad = max_span > 0 ? "%s: %s must not decrease, at most 2^24 points in a problem" : "%s: %s must not decrease";
    if (!bad) return CCAL_OK;
    char msg[160];
    snprintf(msg, sizeof msg, bad, where, name);
    return fail(ctx, CCAL_ERR_INVALID_ARG, msg);
}

class CallBlock : public CallPlan {
    ccal_ctx* ctx;
    char* base = nullptr;
    hipError_t e = hipSuccess;

public:
    explicit CallBlock(ccal_ctx* c) : ctx(c) {}
    CallBlock(const CallBlock&) = delete;
    CallBlock& operator=(const CallBlock&) = delete;
    ~CallBlock() {
        if (!base) return;
        (void)hipStreamSynchronize(ctx->stream);
        ctx_release(ctx, base, false);
    }
    bool ok() const { return e == hipSuccess; }
    void note(hipError_t r) { if (ok()) e = r; }
    bool alloc() {                                   // after the last add(); false: there is no block, leave through finish()
        note(hipSetDevice(ctx->device));
        if (ok()) note(ctx_dev_alloc(ctx, (void**)&base, total));
        return ok();
    }
    template <class T> T* at(Slice<T> s) const { return s.bytes ? reinterpret_cast<T*>(base + s.off) : nullptr; }
    // the test hook's NaN fill over the slices first .. last (slices of doubles, never offsets, indices, seeds or counts)
    template <class A, class B> void poison(Slice<A> first, Slice<B> last) {
        if (ok()) note(test_poison_f64(ctx, base + first.off, last.off + last.bytes - first.off, false, ctx->stream));
    }
    template <class T> void memset(Slice<T> s, int value, size_t count) {
        if (ok() && count) note(hipMemsetAsync(at(s), value, count * sizeof(T), ctx->stream));
    }
    template <class T> void upload(Slice<T> s, const void* host, size_t count) {
        if (ok() && count) note(hipMemcpyAsync(at(s), host, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    }
    template <class T> void download(void* host, const T* dev, size_t count) {       // host == nullptr: an optional output not asked for
        if (ok() && host && count) note(hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    }
    void launched() { note(hipGetLastError()); }
    int finish(const char* where) {
        if (ok()) note(hipStreamSynchronize(ctx->stream));
        return ok() ? CCAL_OK : hip_fail(ctx, where, e);
    }
};

}  // namespace ccal

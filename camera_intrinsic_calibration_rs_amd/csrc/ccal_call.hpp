// One-shot batch calls (host arrays in, host arrays out): ONE device block of the context's allocator, cut into slices that each
// start on a 256-byte boundary; uploads, the launch, downloads and one synchronise, all on the context's stream.
//   CallPlan   the slices in order and the total - plain arithmetic, no context and no HIP call (ccal_plan.hpp; GuardedPlan: with
//              the tests' guards)
//   CallBlock  the plan, the block and a sticky hipError_t: after the first failure every step is a no-op and finish() reports it;
//              the destructor drains the stream before the block goes back to the context's cache, on every way out.  In the tests'
//              guard mode (CCAL_TEST_GUARD_SLICES in the second library) guards of a known byte lie round every slice and
//              finish() reports a damaged one
//   BadArg     the way out of an entry point on a bad argument, with the call's name in the message
//   check_offsets  the argument check of a batched call's CSR offsets, with the call's name in the message
//   GreyBatch  the image arguments of the image stages' calls: their check (its messages, and a source / destination pair's check:
//              ccal_image_plan.hpp), an image's bytes, the device pointer to a chunk's images
//   test_chunk_bytes  the tests' way to make those calls cut a small batch into chunks
// Host only; for the translation units of the one-shot entry points ("One-shot calls").
#pragma once
#include <cstdio>
#include <cstdlib>
#include "ccal_image_plan.hpp"
#include "ccal_internal.hpp"
#include "ccal_plan.hpp"

namespace ccal {

// the two ways out of a one-shot entry point with the context's message set: a status of the caller's choice / CCAL_ERR_HIP "<where>: <HIP's text>"
inline int fail(ccal_ctx* ctx, int code, const char* msg) { note_error(ctx, msg); return code; }
inline int hip_fail(ccal_ctx* ctx, const char* where, hipError_t e) {
    try { ctx->err = std::string(where) + ": " + hipGetErrorString(e); } catch (...) { }
    return CCAL_ERR_HIP;
}
// an entry point's way out on a bad argument: bad("what") is CCAL_ERR_INVALID_ARG with "<where>: <what>" as the context's message
struct BadArg {
    ccal_ctx* ctx; const char* where;
    int operator()(const char* what) const { char msg[160]; snprintf(msg, sizeof msg, "%s: %s", where, what); return fail(ctx, CCAL_ERR_INVALID_ARG, msg); }
};

// offsets[0] == 0, then over the n problems offsets[0 .. n]: no decrease and, with max_span > 0 (2^24, what the kernels index a
// problem by), no problem of more points.  CCAL_OK, or CCAL_ERR_INVALID_ARG with "<where>: <name>..." as the context's message.
inline int check_offsets(ccal_ctx* ctx, const char* where, const char* name, const int64_t* offsets, size_t n, int64_t max_span) {
    const char* bad = offsets[0] != 0 ? "[0] != 0" : nullptr;
    for (size_t i = 0; i < n && !bad; ++i)
        if (offsets[i + 1] < offsets[i] || (max_span > 0 && offsets[i + 1] - offsets[i] > max_span))
            bad = max_span > 0 ? " must not decrease, at most 2^24 points in a problem" : " must not decrease";
    return bad ? BadArg{ ctx, where }((std::string(name) + bad).c_str()) : CCAL_OK;
}

class CallBlock : public GuardedPlan {
    ccal_ctx* ctx;
    char* base = nullptr;
    hipError_t e = hipSuccess;

public:
    explicit CallBlock(ccal_ctx* c) : ctx(c) { guard_front(test_guard_slices() ? kGuardGap : 0); }
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
        fill_guards();
        return ok();
    }
    template <class T> T* at(Slice<T> s) const { return s.bytes ? reinterpret_cast<T*>(base + s.off) : nullptr; }
    // the test hook's NaN fill over the slices first .. last (slices of doubles, never offsets, indices, seeds or counts)
    // In the guard mode the fill spans the guards between its slices without touching them: it goes from guard to guard, so that they
    // hold their pattern after it - and still hold what a kernel of an earlier chunk did to them, which a refill would wipe out.
    template <class A, class B> void poison(Slice<A> first, Slice<B> last) {
        size_t from = first.off;
        const size_t end = last.off + last.bytes;
        for (int i = 0; i < n_guards && ok(); ++i) {
            const Guard& g = guards[i];
            if (g.off + g.bytes <= from || g.off >= end) continue;
            if (g.off > from) note(test_poison_f64(ctx, base + from, g.off - from, false, ctx->stream));
            from = g.off + g.bytes;
        }
        if (ok() && from < end) note(test_poison_f64(ctx, base + from, end - from, false, ctx->stream));
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
        if (ok() && n_guards) return check_guards(where);
        return ok() ? CCAL_OK : hip_fail(ctx, where, e);
    }

private:
    // The guard mode (the second library with CCAL_TEST_GUARD_SLICES=1, tests/test_gpu_guard.py; n_guards == 0 everywhere else): the
    // plan's guards hold kGuardByte from alloc() on, and finish() - a call that got that far without an error - reads them back.
    static constexpr size_t kGuardGap = 256;
    static constexpr int kGuardByte = 0xA5;          // neither a cleared byte nor the poison's 0xFF
    void fill_guards() {
        for (int i = 0; i < n_guards && ok(); ++i) note(hipMemsetAsync(base + guards[i].off, kGuardByte, guards[i].bytes, ctx->stream));
    }
    // the first damaged byte: CCAL_ERR_HIP, "<where>: guard after slice <ordinal> damaged, <d> bytes past the slice's end" or "<where>:
    // guard in front of the block damaged, <d> bytes in front of the first slice"
    int check_guards(const char* where) {
        size_t all = 0;
        for (int i = 0; i < n_guards; ++i) all += guards[i].bytes;
        std::vector<unsigned char> h(all);
        unsigned char* to = h.data();
        for (int i = 0; i < n_guards && ok(); to += guards[i++].bytes)
            note(hipMemcpyAsync(to, base + guards[i].off, guards[i].bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (ok()) note(hipStreamSynchronize(ctx->stream));
        if (!ok()) return hip_fail(ctx, where, e);
        const unsigned char* at = h.data();
        for (int i = 0; i < n_guards; at += guards[i++].bytes) {
            const Guard& g = guards[i];
            for (size_t j = 0; j < g.bytes; ++j) {
                if (at[j] == kGuardByte) continue;
                char msg[200];
                if (g.after < 0) snprintf(msg, sizeof msg, "%s: guard in front of the block damaged, %zu bytes in front of the first slice", where, g.bytes - j);
                else snprintf(msg, sizeof msg, "%s: guard after slice %d damaged, %zu bytes past the slice's end", where, g.after, j);
                return fail(ctx, CCAL_ERR_HIP, msg);
            }
        }
        return CCAL_OK;
    }
};

// A batch of grey images [n_img][height][width] of CCAL_PIX_U8 / CCAL_PIX_U16, in host memory (a _batch entry point) or already on
// the device (_dev).
struct GreyBatch {
    int dtype, width, height, n_img;
    const void* images;
    bool on_device;
    // the message of the first argument out of range, or nullptr (images == NULL is the caller's check: it comes after n_img == 0)
    const char* bad() const { return grey_batch_bad(dtype, width, height, n_img); }
    size_t img_bytes() const { return grey_image_bytes(dtype, width, height); }
    size_t staged_bytes(size_t m) const { return on_device ? 0 : img_bytes() * m; }       // room in the call's block for m images
    // the device pointer to the images k0 .. k0 + m - 1: where they are, or slice s of the block, to which they are uploaded
    const void* chunk(CallBlock& blk, Slice<char> s, size_t k0, size_t m) const {
        const char* first = static_cast<const char*>(images) + k0 * img_bytes();
        if (on_device) return first;
        blk.upload(s, first, img_bytes() * m);
        return blk.at(s);
    }
};

// The block one launch sequence of an image stage should need; larger batches go chunk by chunk.  In the second library only
// (-DCCAL_TEST_HOOKS) the environment variable `env` replaces the limit, so that a test cuts a small batch into chunks
// (test_a_batch_cut_into_chunks of tests/test_gpu_detect.py, test_gpu_quads.py, test_gpu_tags.py, test_gpu_detect_tags.py); read on
// every call.  static: the units of one library are compiled with and without the macro.
static inline size_t test_chunk_bytes(const char* env, size_t dflt) {
#ifdef CCAL_TEST_HOOKS
    if (const char* e = std::getenv(env)) return (size_t)std::strtoull(e, nullptr, 10);
#endif
    (void)env;
    return dflt;
}

}  // namespace ccal

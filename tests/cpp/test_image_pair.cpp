// The argument check of an image-to-image stage's source / destination pair (csrc/ccal_image_plan.hpp: image_pair_check, and
// grey_batch_bad behind GreyBatch::bad) as a plain program: every message, their order when two arguments are bad at once, n_img == 0,
// blocks that touch and blocks that share one byte, an image of more than 2^31 - 1 pixels.  The pointers are numbers: the check only
// compares them.  Prints "OK <checks>" and returns 0, or names the first check that failed (tests/test_image_pair_cpu.py).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../../camera_intrinsic_calibration_rs_amd/csrc/ccal_image_plan.hpp"

namespace {

int n_checks = 0, n_failed = 0;

const void* at(uintptr_t p) { return reinterpret_cast<const void*>(p); }

// what == nullptr: no message is expected, and go says whether the stage is to launch
void expect(int line, const ccal::PairCheck& got, const char* what, bool go) {
    ++n_checks;
    const bool same_what = what ? (got.what && std::strcmp(got.what, what) == 0) : got.what == nullptr;
    if (same_what && got.go == go) return;
    ++n_failed;
    std::printf("line %d: got (%s, %d), expected (%s, %d)\n", line, got.what ? got.what : "-", (int)got.go, what ? what : "-", (int)go);
}
#define EXPECT(call, what, go) expect(__LINE__, call, what, go)

constexpr int U8 = CCAL_PIX_U8, U16 = CCAL_PIX_U16;
const char* const kSrcDtype = "src_dtype is neither CCAL_PIX_U8 nor CCAL_PIX_U16";
const char* const kDstDtype = "dst_dtype is neither CCAL_PIX_U8 nor CCAL_PIX_U16";
const char* const kSize = "a size is not positive";
const char* const kPixels = "more than 2^31 - 1 pixels in an image";
const char* const kSrcNull = "src_dev is NULL";
const char* const kDstNull = "dst_dev is NULL";
const char* const kOverlap = "src_dev and dst_dev overlap";

}  // namespace

int main() {
    using ccal::image_pair_check;
    const uintptr_t A = 1u << 20, B = 1u << 22;                  // far apart
    const void* const src = at(A);
    const void* const dst = at(B);

    // a good call, every pair of types
    for (int s : { U8, U16 })
        for (int d : { U8, U16 }) EXPECT(image_pair_check(s, d, 8, 8, 3, src, dst), nullptr, true);

    // every message on its own
    EXPECT(image_pair_check(2, U8, 8, 8, 1, src, dst), kSrcDtype, false);
    EXPECT(image_pair_check(-1, U8, 8, 8, 1, src, dst), kSrcDtype, false);
    EXPECT(image_pair_check(U8, 2, 8, 8, 1, src, dst), kDstDtype, false);
    EXPECT(image_pair_check(U8, -1, 8, 8, 1, src, dst), kDstDtype, false);
    EXPECT(image_pair_check(U8, U8, 0, 8, 1, src, dst), kSize, false);
    EXPECT(image_pair_check(U8, U8, 8, 0, 1, src, dst), kSize, false);
    EXPECT(image_pair_check(U8, U8, -8, 8, 1, src, dst), kSize, false);
    EXPECT(image_pair_check(U8, U8, 8, 8, -1, src, dst), kSize, false);
    EXPECT(image_pair_check(U8, U8, 8, 8, 1, nullptr, dst), kSrcNull, false);
    EXPECT(image_pair_check(U8, U8, 8, 8, 1, src, nullptr), kDstNull, false);
    EXPECT(image_pair_check(U8, U8, 8, 8, 1, src, src), kOverlap, false);

    // width x height beyond 2^31 - 1 is refused, 2^31 - 1 itself is not: 46341^2 = 2^31 + 4633, 2147483647 x 1, 65536 x 32768 = 2^31
    EXPECT(image_pair_check(U8, U8, 46341, 46341, 1, src, dst), kPixels, false);
    EXPECT(image_pair_check(U16, U8, 65536, 32768, 1, src, dst), kPixels, false);
    EXPECT(image_pair_check(U8, U16, INT32_MAX, INT32_MAX, 0, nullptr, nullptr), kPixels, false);
    EXPECT(image_pair_check(U8, U8, INT32_MAX, 1, 0, nullptr, nullptr), nullptr, false);
    EXPECT(image_pair_check(U8, U8, INT32_MAX, 1, 1, at(uintptr_t(1) << 40), at(uintptr_t(1) << 42)), nullptr, true);

    // two at once: the source's dtype, the sizes, the pixel count, the destination's dtype, src_dev, dst_dev, the overlap - in this order
    EXPECT(image_pair_check(7, 7, 8, 8, 1, src, dst), kSrcDtype, false);
    EXPECT(image_pair_check(7, U8, 0, 8, 1, src, dst), kSrcDtype, false);
    EXPECT(image_pair_check(7, U8, 8, 8, 1, nullptr, nullptr), kSrcDtype, false);
    EXPECT(image_pair_check(U8, 7, 0, 8, 1, src, dst), kSize, false);
    EXPECT(image_pair_check(U8, 7, 46341, 46341, 1, src, dst), kPixels, false);
    EXPECT(image_pair_check(U8, U8, 0, 46341, 1, src, dst), kSize, false);
    EXPECT(image_pair_check(U8, U8, 46341, 46341, -1, src, dst), kSize, false);
    EXPECT(image_pair_check(U8, 7, 8, 8, 1, nullptr, dst), kDstDtype, false);
    EXPECT(image_pair_check(U8, 7, 8, 8, 0, nullptr, nullptr), kDstDtype, false);
    EXPECT(image_pair_check(U8, U8, 0, 8, 1, nullptr, nullptr), kSize, false);
    EXPECT(image_pair_check(U8, U8, 8, 8, 1, nullptr, nullptr), kSrcNull, false);
    EXPECT(image_pair_check(U8, U8, 8, 8, -1, nullptr, nullptr), kSize, false);

    // n_img == 0 is success with nothing to do, and no pointer is looked at: NULL, or one block for both
    for (int s : { U8, U16 })
        for (int d : { U8, U16 }) {
            EXPECT(image_pair_check(s, d, 8, 8, 0, nullptr, nullptr), nullptr, false);
            EXPECT(image_pair_check(s, d, 8, 8, 0, src, src), nullptr, false);
        }

    // overlap.  n images of w x h: the source has sb = es n w h bytes from A, the destination db = ed n w h bytes.  The destination
    // right behind the source (A + sb) or right in front of it (A - db) touches it and passes; one byte nearer either way shares a
    // byte and fails - also where the two blocks differ in length (u8 -> u16, u16 -> u8)
    for (int s : { U8, U16 })
        for (int d : { U8, U16 })
            for (int n : { 1, 3 }) {
                const int w = 8, h = 8;
                const uintptr_t sb = (uintptr_t)(s == U16 ? 2 : 1) * n * w * h, db = (uintptr_t)(d == U16 ? 2 : 1) * n * w * h;
                EXPECT(image_pair_check(s, d, w, h, n, at(A), at(A + sb)), nullptr, true);
                EXPECT(image_pair_check(s, d, w, h, n, at(A), at(A - db)), nullptr, true);
                EXPECT(image_pair_check(s, d, w, h, n, at(A), at(A + sb - 1)), kOverlap, false);
                EXPECT(image_pair_check(s, d, w, h, n, at(A), at(A - db + 1)), kOverlap, false);
                EXPECT(image_pair_check(s, d, w, h, n, at(A), at(A + 1)), kOverlap, false);     // one inside the other
                EXPECT(image_pair_check(s, d, w, h, n, at(A), at(A)), kOverlap, false);
            }
    // the GPU tests' figures: 8 x 8 u8 at +-63 and +-64 bytes, u16 on one side at +-127
    EXPECT(image_pair_check(U8, U8, 8, 8, 1, at(A), at(A + 63)), kOverlap, false);
    EXPECT(image_pair_check(U8, U8, 8, 8, 1, at(A), at(A - 63)), kOverlap, false);
    EXPECT(image_pair_check(U8, U8, 8, 8, 1, at(A), at(A + 64)), nullptr, true);
    EXPECT(image_pair_check(U8, U8, 8, 8, 1, at(A), at(A - 64)), nullptr, true);
    EXPECT(image_pair_check(U16, U8, 8, 8, 1, at(A), at(A + 127)), kOverlap, false);
    EXPECT(image_pair_check(U8, U16, 8, 8, 1, at(A), at(A - 127)), kOverlap, false);

    // the single-batch check behind GreyBatch::bad names plain `dtype`
    ++n_checks;
    const char* one = ccal::grey_batch_bad(2, 8, 8, 1);
    if (!one || std::strcmp(one, "dtype is neither CCAL_PIX_U8 nor CCAL_PIX_U16") != 0) { ++n_failed; std::printf("grey_batch_bad: the dtype message\n"); }
    ++n_checks;
    if (ccal::grey_batch_bad(U16, 8, 8, 0) != nullptr) { ++n_failed; std::printf("grey_batch_bad: a good batch\n"); }

    if (n_failed) { std::printf("FAILED %d of %d\n", n_failed, n_checks); return 1; }
    std::printf("OK %d\n", n_checks);
    return 0;
}

// The argument check of the grey stage (csrc/ccal_image_plan.hpp: grey_stage_check, behind ccal_grey_dev) as a plain program: every
// message, their order when two arguments are bad at once, n_img == 0, blocks that touch and blocks that share one byte - their byte
// counts follow from the layout, the types and the bin -, and a source image of more than 2^31 - 1 pixels.  The pointers are numbers:
// the check only compares them.  Prints "OK <checks>" and returns 0, or names the first check that failed (tests/test_grey_cpu.py).
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
constexpr int GREY = CCAL_LAYOUT_GREY, RGB = CCAL_LAYOUT_RGB, BGRA = CCAL_LAYOUT_BGRA, RGGB = CCAL_LAYOUT_BAYER_RGGB, GBRG = CCAL_LAYOUT_BAYER_GBRG;
const char* const kOpts = "opts is NULL";
const char* const kLayout = "layout is not a ccal_pixel_layout";
const char* const kBin = "bin is not 1, 2 or 4";
const char* const kNegative = "a weight (w_r, w_g, w_b) is negative";
const char* const kSum = "the weights w_r + w_g + w_b do not sum to 65536";
const char* const kSrcDtype = "src_dtype is neither CCAL_PIX_U8 nor CCAL_PIX_U16";
const char* const kDstDtype = "dst_dtype is neither CCAL_PIX_U8 nor CCAL_PIX_U16";
const char* const kSize = "a size is not positive";
const char* const kPixels = "more than 2^31 - 1 pixels in an image";
const char* const kBelowBin = "width or height is below bin";
const char* const kBayerSide = "a Bayer layout needs a width and a height of at least 2";
const char* const kSrcNull = "src_dev is NULL";
const char* const kDstNull = "dst_dev is NULL";
const char* const kOverlap = "src_dev and dst_dev overlap";

ccal_grey_opts opts(int bin = 1, int w_r = 19595, int w_g = 38470, int w_b = 7471) { return ccal_grey_opts{ bin, w_r, w_g, w_b }; }

}  // namespace

int main() {
    using ccal::grey_stage_check;
    const uintptr_t A = uintptr_t(1) << 30, B = uintptr_t(1) << 32;           // far apart
    const void* const src = at(A);
    const void* const dst = at(B);
    const ccal_grey_opts def = opts();

    // a good call: every layout, every pair of types, every bin
    for (int layout = CCAL_LAYOUT_GREY; layout <= CCAL_LAYOUT_BAYER_GBRG; ++layout)
        for (int s : { U8, U16 })
            for (int d : { U8, U16 })
                for (int bin : { 1, 2, 4 }) {
                    const ccal_grey_opts o = opts(bin);
                    EXPECT(grey_stage_check(layout, s, d, 8, 8, 3, src, dst, &o), nullptr, true);
                }

    // every message on its own
    EXPECT(grey_stage_check(RGB, U8, U8, 8, 8, 1, src, dst, nullptr), kOpts, false);
    EXPECT(grey_stage_check(-1, U8, U8, 8, 8, 1, src, dst, &def), kLayout, false);
    EXPECT(grey_stage_check(9, U8, U8, 8, 8, 1, src, dst, &def), kLayout, false);
    for (int bin : { 0, 3, 8, -1 }) {
        const ccal_grey_opts o = opts(bin);
        EXPECT(grey_stage_check(RGB, U8, U8, 8, 8, 1, src, dst, &o), kBin, false);
    }
    {
        const ccal_grey_opts r = opts(1, -1, 65537, 0), g = opts(1, 65537, -1, 0), b = opts(1, 0, 65537, -1);
        EXPECT(grey_stage_check(RGB, U8, U8, 8, 8, 1, src, dst, &r), kNegative, false);
        EXPECT(grey_stage_check(RGB, U8, U8, 8, 8, 1, src, dst, &g), kNegative, false);
        EXPECT(grey_stage_check(RGB, U8, U8, 8, 8, 1, src, dst, &b), kNegative, false);
        const ccal_grey_opts low = opts(1, 19595, 38470, 7470), high = opts(1, 19595, 38470, 7472), zero = opts(1, 0, 0, 0);
        const ccal_grey_opts wrap = opts(1, INT32_MAX, INT32_MAX, 65538);     // 2^32 + 65536: the sum is not taken in 32 bits
        EXPECT(grey_stage_check(RGB, U8, U8, 8, 8, 1, src, dst, &low), kSum, false);
        EXPECT(grey_stage_check(RGB, U8, U8, 8, 8, 1, src, dst, &high), kSum, false);
        EXPECT(grey_stage_check(RGB, U8, U8, 8, 8, 1, src, dst, &zero), kSum, false);
        EXPECT(grey_stage_check(RGB, U8, U8, 8, 8, 1, src, dst, &wrap), kSum, false);
        const ccal_grey_opts red = opts(1, 65536, 0, 0), blue = opts(4, 0, 0, 65536);
        EXPECT(grey_stage_check(RGB, U8, U8, 8, 8, 1, src, dst, &red), nullptr, true);
        EXPECT(grey_stage_check(RGB, U8, U8, 8, 8, 1, src, dst, &blue), nullptr, true);
    }
    EXPECT(grey_stage_check(RGB, 2, U8, 8, 8, 1, src, dst, &def), kSrcDtype, false);
    EXPECT(grey_stage_check(RGB, -1, U8, 8, 8, 1, src, dst, &def), kSrcDtype, false);
    EXPECT(grey_stage_check(RGB, U8, 2, 8, 8, 1, src, dst, &def), kDstDtype, false);
    EXPECT(grey_stage_check(RGB, U8, -1, 8, 8, 1, src, dst, &def), kDstDtype, false);
    EXPECT(grey_stage_check(RGB, U8, U8, 0, 8, 1, src, dst, &def), kSize, false);
    EXPECT(grey_stage_check(RGB, U8, U8, 8, 0, 1, src, dst, &def), kSize, false);
    EXPECT(grey_stage_check(RGB, U8, U8, -8, 8, 1, src, dst, &def), kSize, false);
    EXPECT(grey_stage_check(RGB, U8, U8, 8, 8, -1, src, dst, &def), kSize, false);
    {
        const ccal_grey_opts two = opts(2), four = opts(4);
        EXPECT(grey_stage_check(RGB, U8, U8, 1, 8, 1, src, dst, &two), kBelowBin, false);
        EXPECT(grey_stage_check(RGB, U8, U8, 8, 1, 1, src, dst, &two), kBelowBin, false);
        EXPECT(grey_stage_check(RGB, U8, U8, 3, 8, 1, src, dst, &four), kBelowBin, false);
        EXPECT(grey_stage_check(RGGB, U8, U8, 8, 3, 1, src, dst, &four), kBelowBin, false);
        EXPECT(grey_stage_check(RGB, U8, U8, 2, 2, 1, src, dst, &two), nullptr, true);
        EXPECT(grey_stage_check(RGGB, U8, U8, 4, 4, 1, src, dst, &four), nullptr, true);
    }
    EXPECT(grey_stage_check(RGGB, U8, U8, 1, 8, 1, src, dst, &def), kBayerSide, false);
    EXPECT(grey_stage_check(GBRG, U16, U8, 8, 1, 1, src, dst, &def), kBayerSide, false);
    EXPECT(grey_stage_check(RGGB, U8, U8, 2, 2, 1, src, dst, &def), nullptr, true);
    EXPECT(grey_stage_check(GREY, U8, U8, 1, 1, 1, src, dst, &def), nullptr, true);
    EXPECT(grey_stage_check(BGRA, U16, U8, 1, 1, 1, src, dst, &def), nullptr, true);
    EXPECT(grey_stage_check(RGB, U8, U8, 8, 8, 1, nullptr, dst, &def), kSrcNull, false);
    EXPECT(grey_stage_check(RGB, U8, U8, 8, 8, 1, src, nullptr, &def), kDstNull, false);
    EXPECT(grey_stage_check(RGB, U8, U8, 8, 8, 1, src, src, &def), kOverlap, false);

    // width x height of the SOURCE beyond 2^31 - 1 is refused whatever the bin leaves of it, 2^31 - 1 itself is not
    {
        const ccal_grey_opts four = opts(4);
        EXPECT(grey_stage_check(GREY, U8, U8, 46341, 46341, 1, src, dst, &def), kPixels, false);
        EXPECT(grey_stage_check(RGB, U16, U8, 65536, 32768, 1, src, dst, &four), kPixels, false);
        EXPECT(grey_stage_check(RGGB, U8, U16, INT32_MAX, INT32_MAX, 0, nullptr, nullptr, &def), kPixels, false);
        EXPECT(grey_stage_check(GREY, U8, U8, INT32_MAX, 1, 0, nullptr, nullptr, &def), nullptr, false);
        EXPECT(grey_stage_check(BGRA, U16, U16, INT32_MAX, 1, 1, at(uintptr_t(1) << 44), at(uintptr_t(1) << 40), &def), nullptr, true);
        EXPECT(grey_stage_check(RGGB, U8, U8, 32768, 65535, 1, at(uintptr_t(1) << 44), at(uintptr_t(1) << 40), &four), nullptr, true);
    }

    // two at once: opts, the layout, the bin, a negative weight, the sum, the source's dtype, the sizes, the pixel count, the
    // destination's dtype, the bin against the sizes, the mosaic's sides, src_dev, dst_dev, the overlap - in this order
    {
        const ccal_grey_opts bad_bin = opts(3, -1, 0, 0), neg = opts(1, -1, 0, 0), sum = opts(1, 1, 1, 1), two = opts(2);
        EXPECT(grey_stage_check(-1, 7, 7, 0, 0, -1, nullptr, nullptr, nullptr), kOpts, false);
        EXPECT(grey_stage_check(-1, 7, 7, 0, 0, -1, nullptr, nullptr, &bad_bin), kLayout, false);
        EXPECT(grey_stage_check(RGB, 7, 7, 0, 0, -1, nullptr, nullptr, &bad_bin), kBin, false);
        EXPECT(grey_stage_check(RGB, 7, 7, 0, 0, -1, nullptr, nullptr, &neg), kNegative, false);
        EXPECT(grey_stage_check(RGB, 7, 7, 0, 0, -1, nullptr, nullptr, &sum), kSum, false);
        EXPECT(grey_stage_check(RGB, 7, 7, 0, 0, -1, nullptr, nullptr, &def), kSrcDtype, false);
        EXPECT(grey_stage_check(RGB, U8, 7, 0, 46341, 1, nullptr, nullptr, &def), kSize, false);
        EXPECT(grey_stage_check(RGB, U8, 7, 46341, 46341, 1, nullptr, nullptr, &def), kPixels, false);
        EXPECT(grey_stage_check(RGGB, U8, 7, 1, 1, 1, nullptr, nullptr, &two), kDstDtype, false);
        EXPECT(grey_stage_check(RGGB, U8, U8, 1, 1, 1, nullptr, nullptr, &two), kBelowBin, false);
        EXPECT(grey_stage_check(RGGB, U8, U8, 1, 1, 1, nullptr, nullptr, &def), kBayerSide, false);
        EXPECT(grey_stage_check(RGGB, U8, U8, 1, 1, 0, nullptr, nullptr, &def), kBayerSide, false);
        EXPECT(grey_stage_check(RGGB, U8, U8, 2, 2, 1, nullptr, nullptr, &def), kSrcNull, false);
        EXPECT(grey_stage_check(RGGB, U8, U8, 2, 2, 1, src, nullptr, &def), kDstNull, false);
    }

    // n_img == 0 is success with nothing to do, and no pointer is looked at: NULL, or one block for both
    for (int layout : { GREY, RGB, BGRA, RGGB })
        for (int bin : { 1, 4 }) {
            const ccal_grey_opts o = opts(bin);
            EXPECT(grey_stage_check(layout, U8, U16, 8, 8, 0, nullptr, nullptr, &o), nullptr, false);
            EXPECT(grey_stage_check(layout, U16, U8, 8, 8, 0, src, src, &o), nullptr, false);
        }

    // overlap.  n images of w x h with c channels: the source has sb = es c n w h bytes from A, the destination
    // db = ed n (w / bin) (h / bin) bytes.  The destination right behind the source (A + sb) or right in front of it (A - db) touches it
    // and passes; one byte nearer either way shares a byte and fails.  9 x 7: the bins drop a remainder (4 x 3 and 2 x 1 out)
    struct Combo { int layout, c, s, d, bin; };
    const Combo combos[] = { { GREY, 1, U8, U8, 1 }, { GREY, 1, U16, U8, 2 }, { RGB, 3, U8, U8, 1 }, { RGB, 3, U8, U16, 2 }, { RGB, 3, U16, U8, 4 },
                             { BGRA, 4, U16, U16, 1 }, { BGRA, 4, U8, U16, 4 }, { RGGB, 1, U8, U8, 2 }, { GBRG, 1, U16, U16, 4 }, { RGGB, 1, U8, U16, 1 } };
    for (const Combo& k : combos)
        for (int n : { 1, 3 }) {
            const int w = 9, h = 7;
            const ccal_grey_opts o = opts(k.bin);
            const uintptr_t sb = (uintptr_t)(k.s == U16 ? 2 : 1) * k.c * n * w * h;
            const uintptr_t db = (uintptr_t)(k.d == U16 ? 2 : 1) * n * (w / k.bin) * (h / k.bin);
            EXPECT(grey_stage_check(k.layout, k.s, k.d, w, h, n, at(A), at(A + sb), &o), nullptr, true);
            EXPECT(grey_stage_check(k.layout, k.s, k.d, w, h, n, at(A), at(A - db), &o), nullptr, true);
            EXPECT(grey_stage_check(k.layout, k.s, k.d, w, h, n, at(A), at(A + sb - 1), &o), kOverlap, false);
            EXPECT(grey_stage_check(k.layout, k.s, k.d, w, h, n, at(A), at(A - db + 1), &o), kOverlap, false);
            EXPECT(grey_stage_check(k.layout, k.s, k.d, w, h, n, at(A), at(A + 1), &o), kOverlap, false);     // one inside the other
            EXPECT(grey_stage_check(k.layout, k.s, k.d, w, h, n, at(A), at(A), &o), kOverlap, false);
        }
    // the GPU tests' figures: 8 x 8 RGB u8 (192 bytes) to u8 (64 bytes) at +191 / +192 and -63 / -64
    EXPECT(grey_stage_check(RGB, U8, U8, 8, 8, 1, at(A), at(A + 191), &def), kOverlap, false);
    EXPECT(grey_stage_check(RGB, U8, U8, 8, 8, 1, at(A), at(A + 192), &def), nullptr, true);
    EXPECT(grey_stage_check(RGB, U8, U8, 8, 8, 1, at(A), at(A - 63), &def), kOverlap, false);
    EXPECT(grey_stage_check(RGB, U8, U8, 8, 8, 1, at(A), at(A - 64), &def), nullptr, true);

    if (n_failed) { std::printf("FAILED %d of %d\n", n_failed, n_checks); return 1; }
    std::printf("OK %d\n", n_checks);
    return 0;
}

// The host arithmetic the image stages share: the check of a batch of images and of a source / destination pair, the detector's
// domain, and how ccal_propose_quads_* and ccal_decode_tags_* cut a CSR batch into chunks of whole images.  Plain arithmetic, no context
// and no HIP include, so that plain C++ programs can hold it to the messages and groupings the tests rely on (tests/cpp/test_image_pair.cpp,
// test_grey_check.cpp, test_quads_plan.cpp, through ccal_tagchain_plan.hpp also test_tagchain_plan.cpp; tests/test_image_pair_cpu.py,
// test_grey_cpu.py, test_quads_plan_cpu.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../include/ccal.h"

namespace ccal {

// [n_img][height][width] of CCAL_PIX_U8 / CCAL_PIX_U16: the message of the first argument out of range, `bad_dtype` for the first of
// them, or nullptr (the pointer is the caller's check: it comes after n_img == 0)
inline const char* grey_batch_bad(int dtype, int width, int height, int n_img, const char* bad_dtype = "dtype is neither CCAL_PIX_U8 nor CCAL_PIX_U16") {
    if (dtype != CCAL_PIX_U8 && dtype != CCAL_PIX_U16) return bad_dtype;
    if (width <= 0 || height <= 0 || n_img < 0) return "a size is not positive";
    if ((int64_t)width * height > (int64_t)INT32_MAX) return "more than 2^31 - 1 pixels in an image";
    return nullptr;
}
inline size_t grey_image_bytes(int dtype, int width, int height) { return (dtype == CCAL_PIX_U16 ? 2 : 1) * (size_t)width * (size_t)height; }

// The source and destination blocks of an image-to-image stage (ccal_photo_apply_dev, ccal_normalize_dev).  go: launch; else what is the
// first bad argument's message, or nullptr: nothing to do - n_img == 0 is a success that looks at no pointer.  Blocks that touch are fine.
struct PairCheck { const char* what; bool go; };
inline PairCheck image_pair_check(int src_dtype, int dst_dtype, int width, int height, int n_img, const void* src, const void* dst) {
    if (const char* what = grey_batch_bad(src_dtype, width, height, n_img, "src_dtype is neither CCAL_PIX_U8 nor CCAL_PIX_U16")) return { what, false };
    if (const char* what = grey_batch_bad(dst_dtype, width, height, n_img, "dst_dtype is neither CCAL_PIX_U8 nor CCAL_PIX_U16")) return { what, false };
    if (n_img == 0) return { nullptr, false };
    if (!src) return { "src_dev is NULL", false };
    if (!dst) return { "dst_dev is NULL", false };
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), s1 = s0 + grey_image_bytes(src_dtype, width, height) * (size_t)n_img;
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst), d1 = d0 + grey_image_bytes(dst_dtype, width, height) * (size_t)n_img;
    if (s0 < d1 && d0 < s1) return { "src_dev and dst_dev overlap", false };
    return { nullptr, true };
}

// The grey stage (ccal_grey_dev): a source block of a pixel layout and a destination of another shape, [n_img][height / bin][width / bin].
inline bool layout_is_bayer(int layout) { return layout >= CCAL_LAYOUT_BAYER_RGGB && layout <= CCAL_LAYOUT_BAYER_GBRG; }
inline int layout_channels(int layout) {
    return layout == CCAL_LAYOUT_RGB || layout == CCAL_LAYOUT_BGR ? 3 : layout == CCAL_LAYOUT_RGBA || layout == CCAL_LAYOUT_BGRA ? 4 : 1;
}
// bytes of one source image and of one destination image
inline size_t grey_src_image_bytes(int layout, int dtype, int width, int height) { return (size_t)layout_channels(layout) * grey_image_bytes(dtype, width, height); }
inline size_t grey_dst_image_bytes(int dtype, int width, int height, int bin) { return grey_image_bytes(dtype, width / bin, height / bin); }

// As image_pair_check, for that pair: the options, the layout, then the source's type and sizes, the destination's type, what the bin and
// a mosaic ask of the sizes, and - past n_img == 0 - the pointers and the overlap of the two blocks' bytes.
inline PairCheck grey_stage_check(int layout, int src_dtype, int dst_dtype, int width, int height, int n_img, const void* src, const void* dst,
                                  const ccal_grey_opts* opts) {
    if (!opts) return { "opts is NULL", false };
    if (layout < CCAL_LAYOUT_GREY || layout > CCAL_LAYOUT_BAYER_GBRG) return { "layout is not a ccal_pixel_layout", false };
    if (opts->bin != 1 && opts->bin != 2 && opts->bin != 4) return { "bin is not 1, 2 or 4", false };
    if (opts->w_r < 0 || opts->w_g < 0 || opts->w_b < 0) return { "a weight (w_r, w_g, w_b) is negative", false };
    if ((int64_t)opts->w_r + opts->w_g + opts->w_b != 65536) return { "the weights w_r + w_g + w_b do not sum to 65536", false };
    if (const char* what = grey_batch_bad(src_dtype, width, height, n_img, "src_dtype is neither CCAL_PIX_U8 nor CCAL_PIX_U16")) return { what, false };
    if (dst_dtype != CCAL_PIX_U8 && dst_dtype != CCAL_PIX_U16) return { "dst_dtype is neither CCAL_PIX_U8 nor CCAL_PIX_U16", false };
    if (width < opts->bin || height < opts->bin) return { "width or height is below bin", false };
    if (layout_is_bayer(layout) && (width < 2 || height < 2)) return { "a Bayer layout needs a width and a height of at least 2", false };
    if (n_img == 0) return { nullptr, false };
    if (!src) return { "src_dev is NULL", false };
    if (!dst) return { "dst_dev is NULL", false };
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), s1 = s0 + grey_src_image_bytes(layout, src_dtype, width, height) * (size_t)n_img;
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst), d1 = d0 + grey_dst_image_bytes(dst_dtype, width, height, opts->bin) * (size_t)n_img;
    if (s0 < d1 && d0 < s1) return { "src_dev and dst_dev overlap", false };
    return { nullptr, true };
}

// the pixels the detector tests: x in [d0, d0 + dw), y in [d0, d0 + dh), and their (r+1) x (r+1) blocks, each of which holds at
// most one candidate.  dw == 0: the image is too small to have a domain, there is nothing to launch.
struct DetectDomain {
    int d0 = 0, dw = 0, dh = 0, nbx = 0, nby = 0;
    size_t slots() const { return (size_t)nbx * (size_t)nby; }
};

inline DetectDomain detect_domain(int width, int height, int step, int r) {
    DetectDomain d;
    d.d0 = step + 2;
    if (width <= 2 * d.d0 || height <= 2 * d.d0) return d;
    d.dw = width - 2 * d.d0; d.dh = height - 2 * d.d0;
    d.nbx = (d.dw + r) / (r + 1); d.nby = (d.dh + r) / (r + 1);
    return d;
}

// device bytes of a chunk that grow with it, per row and per image (in the host call an image's pixels come on top):
//   quads  per point the coordinates (2 doubles), the out-edge list (8 indices), degree, count and base; per image its two offsets
//   tags   per quad its corners in and out (2 x 8 doubles), margin and code, reason, id, rot and hamming; per image its offset
constexpr size_t kQuadPerPointBytes = 2 * sizeof(double) + (8 + 3) * sizeof(int32_t), kQuadPerImageBytes = 16;
constexpr size_t kTagPerQuadBytes = (8 + 8 + 1) * sizeof(double) + sizeof(uint64_t) + 4 * sizeof(int32_t), kTagPerImageBytes = 8;

// cut[c] .. cut[c + 1] - 1 are the images of chunk c: as many as keep the chunk within `limit` bytes, at least one; the most images
// and the most rows of a chunk size the call's block
struct ImageChunks {
    std::vector<size_t> cut;
    size_t max_img = 0, max_rows = 0;
};

inline ImageChunks image_chunks(const int64_t* offsets, size_t n_img, size_t per_image, size_t per_row, size_t limit) {
    ImageChunks p;
    p.cut.push_back(0);
    for (size_t k0 = 0; k0 < n_img;) {
        size_t k1 = k0, bytes = 0;
        do {
            bytes += per_image + (size_t)(offsets[k1 + 1] - offsets[k1]) * per_row;
            ++k1;
        } while (k1 < n_img && bytes + per_image + (size_t)(offsets[k1 + 1] - offsets[k1]) * per_row <= limit);
        p.cut.push_back(k1);
        p.max_img = std::max(p.max_img, k1 - k0);
        p.max_rows = std::max(p.max_rows, (size_t)(offsets[k1] - offsets[k0]));
        k0 = k1;
    }
    return p;
}

}  // namespace ccal

// How ccal_detect_tags_* and ccal_detect_checkerboards_* size their device blocks and cut a batch into chunks of whole images: plain
// arithmetic, no context and no HIP include, so that a plain C++ program can hold it to the groupings the tests rely on
// (tests/cpp/test_tagchain_plan.cpp, tests/test_detect_tags_cpu.py).  The counts of an image are not known before its stages have
// run, so the bound per image comes from the caps alone, each cut to what the image's size allows; every image of a call has the same
// bound, and a chunk is a fixed number of images.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include "../../include/ccal.h"
#include "ccal_image_plan.hpp"

namespace ccal {

// device bytes per row of each kind:
//   slot       the detector's (r+1) x (r+1) blocks: pix 4 | hess 12 | resp 8
//   candidate  the detector's stored row 28 (xy 8, hess 12, resp 8) | start / refined xy 16, lambda 8, status 4, iterations 4 |
//              merged xy 16 | compacted point 16 | out-edge list 32, degree, count, base 12
//   quad       indices 16, coordinates 64 | decoded corners 64, margin 8, code 8, reason, id, rot, hamming 16 | the selection's mark 4
//   tag        id, rot, hamming 12 | corners 64 | margin 8
//   image      the detector's Rmax 8 and count 4, three offsets 24, kept / quads / flags / tags / OK quads 20 - rounded up to 64
constexpr size_t kChainPerSlotBytes = 24, kChainPerCandBytes = 136, kChainPerQuadBytes = 180, kChainPerTagBytes = 84, kChainPerImageBytes = 64;
// the board assembly's: per input row xy 16, Hessian 24 or 12, response 8, kept index 4, status 4 in the chain; per kept-row slot
// position 16, M 24, response 8, directions 32, input row 4, links 16, seed 4, attempt bits 4.  In its chain a candidate is the
// detector's stored row and an input row.
constexpr size_t kBoardPerRowBytes = 56, kBoardPerKeptBytes = 108, kBoardPerImageBytes = 64, kBoardChainPerCandBytes = 28 + kBoardPerRowBytes;
constexpr int kBoardMaxKept = CCAL_BOARD_MAX_KEPT;
constexpr size_t kChainChunkBytes = (size_t)256 << 20;    // the block one chunk should need, in either chain and in the assembly's own call
constexpr size_t kChainMaxImages = 65535, kChainQuadsPerPoint = 512;      // a grid's y and z extents; 8^3 chains start at a point

struct ChainShape {
    size_t img_bytes = 0;          // one image
    DetectDomain dom;              // the detector's domain; dw == 0: none, the call has nothing to launch
    size_t slots = 0;              // its (r+1) x (r+1) blocks = the most candidates an image can have
    size_t cand = 0, quads = 0, tags = 0;        // rows per image: the caps, each cut to what can occur
};

inline ChainShape chain_shape(size_t width, size_t height, size_t itemsize, size_t step, size_t r, size_t cand_cap, size_t quad_cap,
                              size_t tag_cap, size_t n_codes) {
    ChainShape s;
    s.img_bytes = itemsize * width * height;
    s.dom = detect_domain((int)width, (int)height, (int)step, (int)r);
    if (!s.dom.dw) return s;
    s.slots = s.dom.slots();
    s.cand = std::min(cand_cap, s.slots);
    s.quads = std::min(quad_cap, kChainQuadsPerPoint * s.cand);
    s.tags = std::min(tag_cap, std::min(s.quads, n_codes));          // an image's tags have distinct ids
    return s;
}

// what both chains begin with (ccal_chain_front.hpp): the image when staged, the detector's slots and row offsets, the candidate rows
inline size_t front_per_image_bytes(bool images_on_device, const ChainShape& s, size_t per_cand) {
    return (images_on_device ? 0 : s.img_bytes) + s.slots * kChainPerSlotBytes + (size_t)s.dom.dh * 4 + s.cand * per_cand;
}

inline size_t chain_per_image_bytes(bool images_on_device, const ChainShape& s) {
    return front_per_image_bytes(images_on_device, s, kChainPerCandBytes) + s.quads * kChainPerQuadBytes + s.tags * kChainPerTagBytes +
           kChainPerImageBytes;
}

// ccal_detect_checkerboards_*: s from chain_shape with quad_cap = tag_cap = n_codes = 1; corners = cols * rows of the board
inline size_t board_chain_per_image_bytes(bool images_on_device, const ChainShape& s, size_t corners) {
    return front_per_image_bytes(images_on_device, s, kBoardChainPerCandBytes) + std::min(s.cand, (size_t)kBoardMaxKept) * kBoardPerKeptBytes +
           corners * 16 + kBoardPerImageBytes;
}

// images per chunk: as many as keep the chunk within `limit` bytes, at least one
inline size_t chain_images_per_chunk(size_t n_img, size_t per_image, size_t limit) {
    return std::min(std::min(n_img, kChainMaxImages), std::max<size_t>(limit / per_image, 1));
}

}  // namespace ccal

// The host arithmetic the image stages share: the detector's domain, and how ccal_propose_quads_* and ccal_decode_tags_* cut a CSR
// batch into chunks of whole images.  Plain arithmetic, no context and no HIP include, so that a plain C++ program can hold it to the
// groupings the tests rely on (tests/cpp/test_quads_plan.cpp, tests/test_quads_plan_cpu.py; through ccal_tagchain_plan.hpp also
// tests/cpp/test_tagchain_plan.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ccal {

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

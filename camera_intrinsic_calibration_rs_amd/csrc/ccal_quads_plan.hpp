// How ccal_propose_quads_* cuts a batch into chunks of whole images: plain arithmetic, no context and no HIP include, so that a
// plain C++ program can hold it to the groupings the tests rely on (tests/cpp/test_quads_plan.cpp, tests/test_quads_plan_cpu.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ccal {

// device bytes of a chunk that grow with it: per point the coordinates (2 doubles), the out-edge list (8 indices), degree, count and
// base; per image its two offsets and, in the host call, its pixels
constexpr size_t kQuadPerPointBytes = 2 * sizeof(double) + (8 + 3) * sizeof(int32_t);
inline size_t quad_per_image_bytes(bool images_on_device, size_t img_bytes) { return (images_on_device ? 0 : img_bytes) + 16; }

// cut[c] .. cut[c + 1] - 1 are the images of chunk c: as many as keep the chunk within `limit` bytes, at least one
inline std::vector<size_t> quad_chunk_cuts(const int64_t* offsets, size_t n_img, size_t per_image, size_t limit) {
    std::vector<size_t> cut(1, 0);
    for (size_t k0 = 0; k0 < n_img;) {
        size_t k1 = k0, bytes = 0;
        do {
            bytes += per_image + (size_t)(offsets[k1 + 1] - offsets[k1]) * kQuadPerPointBytes;
            ++k1;
        } while (k1 < n_img && bytes + per_image + (size_t)(offsets[k1 + 1] - offsets[k1]) * kQuadPerPointBytes <= limit);
        cut.push_back(k1);
        k0 = k1;
    }
    return cut;
}

}  // namespace ccal

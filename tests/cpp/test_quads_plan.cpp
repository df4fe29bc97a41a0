// The chunk planner of ccal_propose_quads_* and ccal_decode_tags_* (csrc/ccal_image_plan.hpp) as a plain program: argv = the stage
// ("quads" / "tags": its byte figures), on_device (0 / 1), image bytes, limit, then the row count of every image; prints
// "PER-POINT <bytes>" (quads) or "PER-QUAD <bytes>" (tags), "CUTS c0 c1 ..." and "MOST <images> <rows>" (tests/test_quads_plan_cpu.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../camera_intrinsic_calibration_rs_amd/csrc/ccal_image_plan.hpp"

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    const bool tags = std::strcmp(argv[1], "tags") == 0;
    if (!tags && std::strcmp(argv[1], "quads") != 0) return 2;
    const bool on_device = std::atoi(argv[2]) != 0;
    const size_t img_bytes = std::strtoull(argv[3], nullptr, 10), limit = std::strtoull(argv[4], nullptr, 10);
    std::vector<int64_t> offsets(1, 0);
    for (int i = 5; i < argc; ++i) offsets.push_back(offsets.back() + std::atoll(argv[i]));
    const size_t per_image = (on_device ? 0 : img_bytes) + (tags ? ccal::kTagPerImageBytes : ccal::kQuadPerImageBytes);
    const size_t per_row = tags ? ccal::kTagPerQuadBytes : ccal::kQuadPerPointBytes;
    const ccal::ImageChunks p = ccal::image_chunks(offsets.data(), offsets.size() - 1, per_image, per_row, limit);
    std::printf("%s %zu\nCUTS", tags ? "PER-QUAD" : "PER-POINT", per_row);
    for (size_t c : p.cut) std::printf(" %zu", c);
    std::printf("\nMOST %zu %zu\n", p.max_img, p.max_rows);
    return 0;
}

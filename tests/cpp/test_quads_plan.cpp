// The chunk planner of ccal_propose_quads_* (csrc/ccal_quads_plan.hpp) as a plain program: argv = on_device (0 / 1), image bytes,
// limit, then the point count of every image; prints "PER-POINT <bytes>" and "CUTS c0 c1 ..." (tests/test_quads_plan_cpu.py).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../camera_intrinsic_calibration_rs_amd/csrc/ccal_quads_plan.hpp"

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const bool on_device = std::atoi(argv[1]) != 0;
    const size_t img_bytes = std::strtoull(argv[2], nullptr, 10), limit = std::strtoull(argv[3], nullptr, 10);
    std::vector<int64_t> offsets(1, 0);
    for (int i = 4; i < argc; ++i) offsets.push_back(offsets.back() + std::atoll(argv[i]));
    const std::vector<size_t> cut = ccal::quad_chunk_cuts(offsets.data(), offsets.size() - 1, ccal::quad_per_image_bytes(on_device, img_bytes), limit);
    std::printf("PER-POINT %zu\nCUTS", ccal::kQuadPerPointBytes);
    for (size_t c : cut) std::printf(" %zu", c);
    std::printf("\n");
    return 0;
}

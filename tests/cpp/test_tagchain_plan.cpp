// The chunk planner of ccal_detect_tags_* and ccal_detect_checkerboards_* (csrc/ccal_tagchain_plan.hpp) as a plain program: argv =
// on_device (0 / 1), width, height, itemsize, step, nms_radius, cand_cap, quad_cap, tag_cap, n_codes, limit, n_img; prints
// "ROWS <slots> <cand> <quads> <tags>", "PER-IMAGE <bytes>" and "CHUNK <images>".  With one more argument, the board's cols * rows,
// also the board chain's "BOARD-PER-IMAGE <bytes>" and "BOARD-CHUNK <images>" (tests/test_detect_tags_cpu.py).
#include <cstdio>
#include <cstdlib>
#include "../../camera_intrinsic_calibration_rs_amd/csrc/ccal_tagchain_plan.hpp"

int main(int argc, char** argv) {
    if (argc != 13 && argc != 14) return 2;
    size_t v[14];
    for (int i = 1; i < argc; ++i) v[i] = std::strtoull(argv[i], nullptr, 10);
    const ccal::ChainShape s = ccal::chain_shape(v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10]);
    const size_t per = ccal::chain_per_image_bytes(v[1] != 0, s);
    std::printf("ROWS %zu %zu %zu %zu\nPER-IMAGE %zu\nCHUNK %zu\n", s.slots, s.cand, s.quads, s.tags, per,
                ccal::chain_images_per_chunk(v[12], per, v[11]));
    if (argc == 14) {
        const size_t board = ccal::board_chain_per_image_bytes(v[1] != 0, s, v[13]);
        std::printf("BOARD-PER-IMAGE %zu\nBOARD-CHUNK %zu\n", board, ccal::chain_images_per_chunk(v[12], board, v[11]));
    }
    return 0;
}

// Shared by ccal_kernels_rdh.hip (kernels) and ccal_init.hip (C ABI): the argument block of the RANSAC launch.
#pragma once
#include <climits>
#include <cstdint>
#include <hip/hip_runtime.h>

namespace ccal {

constexpr int RDH_LDS_PAIRS = 1024;          // pairs of one problem staged in LDS (32 KiB); larger problems read global memory

struct RdhPartial { double score, lambda, H[9]; int32_t idx, n_valid; };     // a workgroup's winner

struct RdhArgs {
    const int64_t* pair_off;     // [n_prob + 1]
    const double* pairs;         // [n_pairs_total][4]  x, y, x', y' (normalised)
    const uint64_t* seeds;       // [n_prob]
    int32_t n_hyp, n_blocks;     // n_blocks = ceil(n_hyp / 64) workgroups per problem
    RdhPartial* part;            // [n_prob][n_blocks]
    double* out_lambda; double* out_H; double* out_score; int32_t* out_idx; int32_t* out_nvalid;     // [n_prob] (H: [n_prob][9])
    int32_t* h_sample; double* h_lambda; double* h_H; double* h_score;       // per hypothesis [n_prob][n_hyp](...), or NULL
};

hipError_t launch_rdh(const RdhArgs& a, int n_prob, int max_pairs, hipStream_t s);

}  // namespace ccal

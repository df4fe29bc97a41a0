// Launch decisions of the Gram and eval launchers, on the host alone (plain C++17: no HIP type, no context): which instantiation a
// run-time (model, focal mode, ...) key or lane mapping selects, how many lanes a frame gets, and whether a launch eliminates its frames'
// pose blocks in its tail.  The launchers (ccal_kernels_fused.hip, ccal_kernels_gram2.hip, ccal_kernels_normal.hip, ccal_kernels_eval.hip)
// hold the kernels and the callables; tests/cpp/test_gram_plan.cpp holds this file against the decisions on record.
#pragma once
#include <algorithm>
#include <cstdint>
#include <type_traits>

#ifndef CCAL_GRAMV_WPB
#define CCAL_GRAMV_WPB 2          // wavefronts per workgroup of the register Gram kernels
#endif

namespace ccal {

// ---- dispatch: run-time keys -> compile-time tags ---------------------------------------------------------------------------------
// f is a generic callable; it gets its arguments as std::integral_constant tags (decltype(tag)::value is a constant expression) and
// every instantiation of it returns R.  A model id outside 0 .. 3 (kUCM .. kOCV5, ccal_models.hpp) gives `invalid` without calling f.
template <int V> using IntTag = std::integral_constant<int, V>;
template <bool V> using BoolTag = std::bool_constant<V>;

template <class R, class F>
R dispatch_model_focal(int model, bool one_focal, R invalid, F&& f) {
    switch (model) {
        case 0: return one_focal ? f(IntTag<0>(), BoolTag<true>()) : f(IntTag<0>(), BoolTag<false>());
        case 1: return one_focal ? f(IntTag<1>(), BoolTag<true>()) : f(IntTag<1>(), BoolTag<false>());
        case 2: return one_focal ? f(IntTag<2>(), BoolTag<true>()) : f(IntTag<2>(), BoolTag<false>());
        case 3: return one_focal ? f(IntTag<3>(), BoolTag<true>()) : f(IntTag<3>(), BoolTag<false>());
        default: return invalid;
    }
}
// the same with a third flag (the eval and matrix-core Gram kernels: a camera other than the reference camera)
template <class R, class F>
R dispatch_model_focal_other(int model, bool one_focal, bool other, R invalid, F&& f) {
    return dispatch_model_focal(model, one_focal, invalid, [&](auto m, auto of) {
        return other ? f(m, of, BoolTag<true>()) : f(m, of, BoolTag<false>());
    });
}
// the lane mappings the register Gram kernels are instantiated for; anything else gives `no_mapping` without calling f
constexpr int kLaneMappings[6] = { 64, 32, 16, 12, 8, 6 };
constexpr bool is_lane_mapping(int lpf) { for (int c : kLaneMappings) if (lpf == c) return true; return false; }
template <class R, class F>
R dispatch_lanes(int lpf, R no_mapping, F&& f) {
    switch (lpf) {
        case 6: return f(IntTag<6>());
        case 8: return f(IntTag<8>());
        case 12: return f(IntTag<12>());
        case 16: return f(IntTag<16>());
        case 32: return f(IntTag<32>());
        case 64: return f(IntTag<64>());
        default: return no_mapping;
    }
}

// ---- lanes per frame ------------------------------------------------------------------------------------------------------------------
// Few lanes = many corner passes per lane but fewer wavefronts, and a wavefront's prologue, reductions and (fused) elimination
// amortised over more corners.  Cost of a launch in units of one corner pass (~1.75 us):
//   one wavefront per SIMD:   rounds x (c0 + passes),   rounds = ceil(wavefronts / 1 024)
//   two wavefronts per SIMD:  g(n) x (c0 + passes),     n = wavefronts / 1 024 SIMDs,
//     g = 1 (n <= 1: every wavefront alone on its SIMD), 1 + 0.3 (n - 1) up to n = 2 (the younger partner runs at ~0.57 of
//     the solo speed until it is alone), 0.65 + 0.43 n beyond (wavefronts past 2 048 wait for a slot: a step at n = 2, then
//     pipelined) - fitted to tools/sweep_lpf.py with the fused elimination (6 / 8 / 12 / 16 / 32 / 64 lanes, 1 500-50 000 frames;
//     EUCM us per build, best in brackets: 5 000 frames 37.4 40.2 33.7 [31.2] 37.2 50.7; 10 000: 52.9 45.8 [40.8] 45.7 58.3 82.4;
//     20 000: 85.2 [67.6] 72.1 74.6 98.0 117; 50 000: 159 [138] 151 154 191 267;  KB4 (k_gram1v) 10 000: [54.6] 78.1 63.4 74.3
//     88.4 138; 20 000: [99.4] 115 116 120 168 214).
// c0 = the prologue + reductions + elimination of a wavefront, in passes, per kernel family:
//   k_gram1v / k_gram1w: 6 (6 lanes: 8).
//   k_gram2, single camera: 6 (6 lanes: 7)
//     (20 000 frames, whole build: 6 lanes 55.1 us, 8: 59.1, 12: 63.8; 50 000 frames: 133.8, 123.5, 136.8).
//   k_gram2, general loop: 7 (6 lanes: 8).  Its launches have no elimination in their tail (two EUCM cameras x 10 000 frames in one
//     launch, whole build: 6 lanes 77.0 us, 8: 81.5, 12: 83.1, 16: 85.0) - but what they measure at 20 000 frames is a larger fixed
//     cost per wavefront (the record goes to HBM, the occupancy term is optimistic beyond four wavefronts per SIMD).
struct LaneCost { bool two_per_simd; double c0_six, c0; };
constexpr LaneCost gram1_lane_cost(bool two_per_simd) { return { two_per_simd, 8.0, 6.0 }; }
constexpr LaneCost gram2_lane_cost(bool two_per_simd, bool gen) { return { two_per_simd, gen ? 8.0 : 7.0, gen ? 7.0 : 6.0 }; }
constexpr int64_t kNoWaveCap = (int64_t)1 << 40;
// `forced` overrides where it is a mapping (developer switches of the second library: CCAL_GRAMV_LPF, FusedArgs::lpf_force); anything
// else would make the launcher's wavefront count and its kernel disagree and is ignored.  Mappings whose wavefronts, rounded to the
// workgroup, would not fit the rows of the partial-sum buffer (`max_waves`: the single-camera loop's fused elimination writes one row
// per wavefront) are left out; six lanes per frame (the fewest wavefronts) always fit (fused_ws_ensure sizes the buffer for them).
// `share`: side-by-side sessions (ccal_solve_batch) share the chip.
inline int lanes_per_frame(int n_obs, int avg_corners, LaneCost k, int forced, int64_t max_waves, int share) {
    if (is_lane_mapping(forced)) return forced;
    const int simds = std::max(1024 / std::max(share, 1), 64);
    int best = 6;
    double best_cost = 1e300;
    for (int lpf : kLaneMappings) {
        const int g = 64 / lpf;
        const int64_t waves = ((int64_t)n_obs + g - 1) / g;
        if ((waves + CCAL_GRAMV_WPB - 1) / CCAL_GRAMV_WPB * CCAL_GRAMV_WPB > max_waves && lpf != 6) continue;
        const int passes = (std::max(avg_corners, 1) + lpf - 1) / lpf;
        const double nw = (double)waves / (double)simds;
        const double occ = !k.two_per_simd ? (double)((waves + simds - 1) / simds)
                                           : (nw <= 1.0 ? 1.0 : (nw <= 2.0 ? 1.0 + 0.3 * (nw - 1.0) : 0.65 + 0.43 * nw));
        const double cost = occ * ((lpf == 6 ? k.c0_six : k.c0) + passes);
        if (cost < best_cost) { best_cost = cost; best = lpf; }        // ties: the wider mapping (listed first)
    }
    return best;
}

// ---- fused elimination ----------------------------------------------------------------------------------------------------------------
// Single-camera loop: the launch eliminates its frames' pose blocks in its tail where that is allowed (fuse_elim) and its wavefronts,
// rounded to the workgroup, fit the rows of the partial-sum buffer (one row per wavefront); n_part = those rows (0: not fused).
// (every size: 300 / 625 / 1 000 / 1 280 frames GN 0.135-0.155 ms fused against 0.145-0.172 with a separate elimination launch and
// the head's own reduction of its <= 40 rows; the second library's CCAL_FUSE_ELIM=0 still takes the separate launch)
// A value that is no lane mapping is not planned for: not fused (dispatch_lanes then refuses the launch).
struct FusePlan { bool fuse; int n_part; };
inline FusePlan fuse_plan(int lpf, int n_obs, bool fuse_elim, int part_cap, bool gen) {
    if (!is_lane_mapping(lpf)) return { false, 0 };
    const int g = 64 / lpf, waves = ((n_obs + g - 1) / g + CCAL_GRAMV_WPB - 1) / CCAL_GRAMV_WPB * CCAL_GRAMV_WPB;
    const bool fuse = !gen && fuse_elim && waves <= part_cap;
    return { fuse, fuse ? waves : 0 };
}

// ---- single-launch groups on k_gram2i ---------------------------------------------------------------------------------------------
// Where the form applies: all wavefronts resident at once (at most 2 048, of 12 lanes = five frames each) in at most 256 workgroups of
// eight - and at least 224 of them (ccal_kernels_gram2.hip: launch_gram2_iter): 1 785 .. 2 048 wavefronts, 8 921 .. 10 240 frames.
constexpr int kG2IterWpb = 8, kG2IterLpf = 12;
inline bool g2_iter_applies(int n_obs) {
    const int g = 64 / kG2IterLpf;
    const int64_t waves = ((int64_t)n_obs + g - 1) / g, wgs = (waves + kG2IterWpb - 1) / kG2IterWpb;
    return waves <= 2048 && wgs <= 256 && wgs >= 224;
}

}  // namespace ccal

// The launch decisions of the Gram and eval launchers (csrc/ccal_gram_plan.hpp) on the host alone - no context, no HIP call.
// argv[1]: the rows of tests/golden/gram_lane_plans.json, flattened by the caller (tests/test_gram_plan_cpu.py), one per line:
//   kernel (1: k_gram1v / k_gram1w, 2: k_gram2)  two_per_simd  general  n_obs  avg_corners  share  max_waves  forced  pick
//   fuse, n_part with fuse_elim = 0   fuse, n_part with fuse_elim = 1      (fuse = -1: a forced-mapping row, the pick alone)
// The table holds what the launchers decided before they shared one cost model; the first row that differs fails the run.
#include <climits>
#include <cstdio>
#include <cstdlib>

#include "../../camera_intrinsic_calibration_rs_amd/csrc/ccal_gram_plan.hpp"

static int bad(const char* what) { std::printf("PLAN-FAIL %s\n", what); return 1; }

static int check_rows(const char* path, long* n_rows) {
    std::FILE* f = std::fopen(path, "r");
    if (!f) return bad("cannot open the rows");
    int kernel, two, gen, n_obs, avg, share, forced, pick, fuse[2], n_part[2];
    long long max_waves;
    int rc = 0;
    while (std::fscanf(f, "%d %d %d %d %d %d %lld %d %d %d %d %d %d", &kernel, &two, &gen, &n_obs, &avg, &share, &max_waves, &forced, &pick,
                       &fuse[0], &n_part[0], &fuse[1], &n_part[1]) == 13) {
        ++*n_rows;
        const ccal::LaneCost cost = kernel == 1 ? ccal::gram1_lane_cost(two != 0) : ccal::gram2_lane_cost(two != 0, gen != 0);
        const int got = ccal::lanes_per_frame(n_obs, avg, cost, forced, max_waves, share);
        bool ok = got == pick && ccal::is_lane_mapping(got);
        ccal::FusePlan fp[2] = { { false, 0 }, { false, 0 } };
        for (int fe = 0; fe < 2 && ok && fuse[0] >= 0; ++fe) {
            fp[fe] = ccal::fuse_plan(got, n_obs, fe != 0, (int)std::min<long long>(max_waves, INT_MAX), gen != 0);
            ok = (int)fp[fe].fuse == fuse[fe] && fp[fe].n_part == n_part[fe];
        }
        if (!ok) {
            std::printf("row %ld: kernel %d two_per_simd %d general %d n_obs %d avg_corners %d share %d max_waves %lld forced %d\n"
                        "  recorded: %d lanes, fuse %d / %d, n_part %d / %d\n  now:      %d lanes, fuse %d / %d, n_part %d / %d\n",
                        *n_rows, kernel, two, gen, n_obs, avg, share, max_waves, forced, pick, fuse[0], fuse[1], n_part[0], n_part[1],
                        got, (int)fp[0].fuse, (int)fp[1].fuse, fp[0].n_part, fp[1].n_part);
            rc = bad("lane mapping or fusion plan differs from the table");
            break;
        }
    }
    if (!rc && !std::feof(f)) rc = bad("malformed row");
    std::fclose(f);
    return rc;
}

// every key reaches exactly its own instantiation: the probes return their compile-time arguments packed into an integer
static int check_dispatch() {
    for (int model = -1; model <= 4; ++model)
        for (int of = 0; of < 2; ++of) {
            const bool valid = model >= 0 && model < 4;
            const int got2 = ccal::dispatch_model_focal(model, of != 0, -1, [](auto m, auto f) { return 100 + decltype(m)::value * 10 + (decltype(f)::value ? 1 : 0); });
            if (got2 != (valid ? 100 + model * 10 + of : -1)) return bad("dispatch_model_focal");
            for (int other = 0; other < 2; ++other) {
                const int got3 = ccal::dispatch_model_focal_other(model, of != 0, other != 0, -1, [](auto m, auto f, auto o) {
                    return 1000 + decltype(m)::value * 100 + (decltype(f)::value ? 10 : 0) + (decltype(o)::value ? 1 : 0);
                });
                if (got3 != (valid ? 1000 + model * 100 + of * 10 + other : -1)) return bad("dispatch_model_focal_other");
            }
        }
    for (int lpf = -1; lpf <= 130; ++lpf) {
        const bool mapping = lpf == 6 || lpf == 8 || lpf == 12 || lpf == 16 || lpf == 32 || lpf == 64;      // (0, 7, 10, 20, ...: none)
        if (ccal::dispatch_lanes(lpf, -1, [](auto l) { return (int)decltype(l)::value; }) != (mapping ? lpf : -1)) return bad("dispatch_lanes");
        if (ccal::is_lane_mapping(lpf) != mapping) return bad("is_lane_mapping");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) return bad("usage");
    if (int rc = check_dispatch()) return rc;
    // k_gram2i's single-launch groups: 12 lanes = 5 frames per wavefront, 224 .. 256 workgroups of eight, at most 2 048 wavefronts
    // -> 1 785 .. 2 048 wavefronts = 8 921 .. 10 240 frames
    if (ccal::g2_iter_applies(0) || ccal::g2_iter_applies(8920) || !ccal::g2_iter_applies(8921) || !ccal::g2_iter_applies(10240) || ccal::g2_iter_applies(10241))
        return bad("g2_iter_applies");
    // a value that is no mapping is not planned for (and not divided by)
    for (int lpf : { 0, 7, 10, 20, -6 }) { const ccal::FusePlan fp = ccal::fuse_plan(lpf, 625, true, 1 << 20, false); if (fp.fuse || fp.n_part != 0) return bad("fuse_plan of no mapping"); }
    long n_rows = 0;
    if (int rc = check_rows(argv[1], &n_rows)) return rc;
    std::printf("PLAN-OK %ld rows\n", n_rows);
    return 0;
}

// The planning part of the one-shot calls' device block (csrc/ccal_call.hpp: CallPlan) on the host alone - no context, no HIP call.
// argv[1], argv[2]: the refine layout's total for np = 5, n_tot = 195 with and without err_out, worked out by the caller
// (tests/test_call_block_cpu.py) from the byte formulas the entry point used before it had a plan.
#include <cstdio>
#include <cstdlib>

#include "../../camera_intrinsic_calibration_rs_amd/csrc/ccal_call.hpp"

using ccal::CallPlan;

static int bad(const char* what) { std::printf("PLAN-FAIL %s\n", what); return 1; }

// slices in declaration order, each on a 256-byte boundary, none overlapping, the total the sum of the rounded sizes
template <class S> static bool follows(const S& s, size_t& end, size_t want_bytes) {
    const bool ok = s.off % 256 == 0 && s.off == end && s.bytes == want_bytes;
    end = s.off + s.bytes;
    return ok;
}

static size_t refine_total(size_t np, size_t n_tot, bool err_out) {
    CallPlan p;
    p.add<int64_t>(np + 1); p.add<double>((n_tot + 1) * 3); p.add<double>((n_tot + 1) * 2); p.add<double>(np * 8);
    p.add<double>(err_out ? n_tot + 1 : 0); p.add<int32_t>(np * 3);
    return p.total;
}

int main(int argc, char** argv) {
    if (argc != 3) return bad("usage");
    for (size_t b : { 0, 1, 255, 256, 257, 511, 512 })
        if (CallPlan::up256(b) != (b + 255) / 256 * 256) return bad("up256");
    CallPlan p;
    size_t end = 0;
    const auto a = p.add<int64_t>(6);          // 48 bytes
    const auto b = p.add<double>(32);          // exactly 256
    const auto none = p.add<double>(0);        // an optional output that was not asked for
    const auto c = p.add<uint8_t>(257);
    const auto d = p.add<int32_t>(1);
    if (!follows(a, end, 256) || !follows(b, end, 256) || !follows(none, end, 0) || !follows(c, end, 512) || !follows(d, end, 256)) return bad("slices");
    if (p.total != end || p.total != 1280) return bad("total");
    if (refine_total(5, 195, true) != std::strtoull(argv[1], nullptr, 10)) return bad("refine layout with err_out");
    if (refine_total(5, 195, false) != std::strtoull(argv[2], nullptr, 10)) return bad("refine layout without err_out");
    std::printf("PLAN-OK %zu %zu\n", refine_total(5, 195, true), refine_total(5, 195, false));
    return 0;
}

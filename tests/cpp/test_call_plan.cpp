// The planning part of the one-shot calls' device block (csrc/ccal_call.hpp: CallPlan) on the host alone - no context, no HIP call.
// argv[1], argv[2]: the refine layout's total for np = 5, n_tot = 195 with and without err_out, worked out by the caller
// (tests/test_call_block_cpu.py) from the byte formulas the entry point used before it had a plan.
#include <cstdio>
#include <cstdlib>

#include "../../camera_intrinsic_calibration_rs_amd/csrc/ccal_call.hpp"

using ccal::CallPlan;
using ccal::GuardedPlan;

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

// The guarded layout (GuardedPlan::guard_front(gap), the tests' CCAL_TEST_GUARD_SLICES): the block begins with a guard of `gap` bytes; a
// present slice starts on a 256-byte boundary right behind the guard in front of it, and its own guard starts at its EXACT end, is at
// least `gap` >= 256 bytes and ends on the next slice's start; an absent slice adds nothing; the total is the sum.
static const char* guarded_layout() {
    const size_t gap = 256;
    GuardedPlan p;
    p.guard_front(gap);
    if (p.total != gap || p.n_guards != 1 || p.guards[0].off != 0 || p.guards[0].bytes != gap || p.guards[0].after != -1) return "front guard";
    const size_t counts[] = { 6, 32, 0, 257, 1, 0, 65 };           // of int64, double, double, uint8, int32, int32, int32
    const size_t sizes[] = { 8, 8, 8, 1, 4, 4, 4 };
    size_t offs[7], rounded[7];
    { const auto s = p.add<int64_t>(counts[0]); offs[0] = s.off; rounded[0] = s.bytes; }
    { const auto s = p.add<double>(counts[1]); offs[1] = s.off; rounded[1] = s.bytes; }
    { const auto s = p.add<double>(counts[2]); offs[2] = s.off; rounded[2] = s.bytes; }
    { const auto s = p.add<uint8_t>(counts[3]); offs[3] = s.off; rounded[3] = s.bytes; }
    { const auto s = p.add<int32_t>(counts[4]); offs[4] = s.off; rounded[4] = s.bytes; }
    { const auto s = p.add<int32_t>(counts[5]); offs[5] = s.off; rounded[5] = s.bytes; }
    { const auto s = p.add<int32_t>(counts[6]); offs[6] = s.off; rounded[6] = s.bytes; }
    size_t end = gap, sum = gap;
    int g = 1;
    for (int i = 0; i < 7; ++i) {
        const size_t exact = counts[i] * sizes[i];
        if (rounded[i] != CallPlan::up256(exact) || offs[i] != end) return "a guarded slice's place";
        if (!exact) continue;                                     // absent: no room, no guard
        if (offs[i] % 256) return "a guarded slice's boundary";
        if (g >= p.n_guards) return "a guard is missing";
        const GuardedPlan::Guard& gd = p.guards[g++];
        if (gd.after != i || gd.off != offs[i] + exact || gd.bytes < gap || gd.bytes != rounded[i] - exact + gap) return "a guard's place";
        end = gd.off + gd.bytes;
        sum += rounded[i] + gap;
    }
    if (g != p.n_guards || p.n_guards != 6 || p.n_slices != 7) return "the guards' count";
    if (p.total != end || p.total != sum) return "the guarded total";
    GuardedPlan q;                                                // gap 0: CallPlan's numbers
    q.guard_front(0);
    q.add<int64_t>(6); q.add<double>(0); q.add<uint8_t>(257);
    if (q.total != 768 || q.n_guards != 0) return "gap 0";
    return nullptr;
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
    if (const char* what = guarded_layout()) return bad(what);
    if (refine_total(5, 195, true) != std::strtoull(argv[1], nullptr, 10)) return bad("refine layout with err_out");
    if (refine_total(5, 195, false) != std::strtoull(argv[2], nullptr, 10)) return bad("refine layout without err_out");
    std::printf("PLAN-OK %zu %zu\n", refine_total(5, 195, true), refine_total(5, 195, false));
    return 0;
}

// The layouts of the persistent blocks (csrc: ProblemLayout, FusedLayout, GeneralLayout, NormalBaseLayout, PoseScratch,
// StatsScratch) on the host alone - no context, no HIP call.
//   golden   prints, as JSON, every slice offset and the total of the problem block and of the fused workspace's two blocks for a fixed
//            list of sizes; tests/test_ws_layouts_cpu.py compares it with tests/golden/ws_layouts.json
//   check    the general workspace and the scratch layouts have no earlier layout to equal: their properties, over rigs of 2, 3, 5 and 8
//            cameras x k_schurq on / off x merged / per-camera Gram lists x with / without sorted lists x n_obs = 0; prints LAYOUT-OK
//   general  <n_slots> <n_obs>: the general block's total for a two-camera EUCM rig under k_schurq (the window of
//            tests/test_gpu_poison.py::test_dirty_general_block_serves_next_rig)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../camera_intrinsic_calibration_rs_amd/csrc/ccal_fused.hpp"

using namespace ccal;

struct Case { const char* name; int n_cams; size_t n_obs, n_slots, n_corners; size_t cam_obs[8]; size_t bin_tab; int K; };       // K = 0: problem block only
static const Case kCases[] = {
    { "empty", 1, 0, 0, 0, { 0 }, 0, 6 },
    { "one_frame", 1, 1, 1, 144, { 1 }, 0, 6 },
    { "ragged600_eucm", 1, 600, 600, 50731, { 600 }, 600 * 4 + 4, 6 },
    { "uniform2000_kb4", 1, 2000, 2000, 288000, { 2000 }, 0, 8 },
    { "ocv5_10000_one_focal", 1, 10000, 10000, 1440000, { 10000 }, 0, 8 },
    { "poses_at_spread_limit", 1, 5461, 5461, 786384, { 5461 }, 0, 6 },
    { "poses_over_spread_limit", 1, 5462, 5462, 786528, { 5462 }, 0, 6 },
    { "rig2", 2, 2040, 1200, 293760, { 1030, 1010 }, 0, 0 },
    { "rig8", 8, 313, 40, 31307, { 40, 40, 39, 40, 38, 40, 39, 37 }, 0, 0 },
};

static bool first;
static void kv(const char* k, size_t v) { std::printf("%s\"%s\": %zu", first ? "" : ", ", k, v); first = false; }
static void ranges(const CallPlan& pl) {
    std::printf(", \"poison\": [");
    for (int i = 0; i < pl.n_poison; ++i) std::printf("%s[%zu, %zu]", i ? ", " : "", pl.poison[i].off, pl.poison[i].bytes);
    std::printf("]");
}

static int golden() {
    std::printf("{\n");
    bool c0 = true;
    for (const Case& c : kCases) {
        std::printf("%s \"%s\": {\"problem\": {", c0 ? "" : ",\n", c.name); c0 = false; first = true;
        const ProblemLayout p(c.n_corners, c.n_obs, c.n_slots, c.n_cams, c.cam_obs, c.bin_tab);
        kv("x", p.x.off); kv("y", p.y.off); kv("z", p.z.off); kv("u", p.u.off); kv("v", p.v.off);
        kv("obs_off", p.obs_off.off); kv("joff", p.joff.off); kv("obs_cam", p.obs_cam.off); kv("obs_slot", p.obs_slot.off);
        for (int k = 0; k < c.n_cams; ++k) { char nm[16]; std::snprintf(nm, sizeof nm, "cam_obs%d", k); kv(nm, p.cam_obs[k].off); }
        kv("bin_tab_bytes", p.bin_tab.bytes); kv("bin_tab", p.bin_tab.off); kv("uploaded", p.uploaded);
        kv("intr", p.intr.off); kv("poses", p.poses.off); kv("extr", p.extr.off);
        kv("intr_c", p.intr_c.off); kv("poses_c", p.poses_c.off); kv("extr_c", p.extr_c.off); kv("total", p.plan.total);
        if (p.plan.zero_bytes || p.plan.n_poison) return 1;        // (cleared as a whole by ccal_problem_create; inputs are never poisoned)
        std::printf("}");
        if (c.K) {
            const FusedLayout f(c.n_slots, c.n_obs, (size_t)pf_size(c.K), (size_t)praw_size(c.K), (size_t)fused_red_size(c.K), (size_t)fused_partial_rows((int)c.n_obs));
            std::printf(", \"fused_dev\": {"); first = true;
            kv("pf0", f.pf[0].off); kv("pf1", f.pf[1].off); kv("praw0", f.praw[0].off); kv("praw1", f.praw[1].off);
            kv("partial", f.partial.off); kv("red", f.red.off); kv("red_stride", f.red_stride); kv("done_cnt", f.done_cnt.off);
            kv("mc_f", f.mc_f.off); kv("cost_f", f.cost_f.off); kv("state", f.state.off); kv("d_stage", f.d_stage.off);
            kv("zero_bytes", f.dev.zero_bytes); ranges(f.dev); kv("total", f.dev.total);
            std::printf("}, \"fused_host\": {"); first = true;
            kv("h_status", f.h_status.off); kv("h_result", f.h_result.off); kv("h_result_bytes", f.h_result.bytes); kv("h_stage", f.h_stage.off);
            ranges(f.host); kv("total", f.host.total);
            if (f.host.zero_bytes != f.h_result.off) return 1;     // h_status alone starts as zeros
            std::printf("}");
        }
        std::printf("}");
    }
    std::printf("\n}\n");
    return 0;
}

// ---- properties
struct Decl { size_t off, bytes, want; unsigned flags; };          // want: the slice's bytes before rounding
template <class T> static Decl decl(Slice<T> s, size_t count, unsigned flags = 0) { return { s.off, s.bytes, count * sizeof(T), flags }; }
static int bad(const char* what, const char* which) { std::printf("LAYOUT-FAIL %s: %s\n", which, what); return 1; }

// every slice on a 256-byte boundary, in declaration order, none overlapping; absent <=> zero bytes; the zero range exactly the union
// of the cleared slices; every poison range inside slices of doubles, each of them covered once; the total the sum of the rounded sizes
static int check(const char* which, const CallPlan& pl, const std::vector<Decl>& ds) {
    size_t end = 0, zero_end = 0;
    std::vector<CallPlan::Range> runs;
    for (const Decl& d : ds) {
        if (d.off % 256 || d.off != end) return bad("a slice is not where the one before it ends, on a 256-byte boundary", which);
        if (d.bytes != (d.want + 255) / 256 * 256 || (d.want == 0) != (d.bytes == 0)) return bad("a slice's room", which);
        if (d.flags & kCleared) { if (d.off != zero_end) return bad("a cleared slice behind one that is not", which); zero_end = d.off + d.bytes; }
        if ((d.flags & kDoubles) && d.bytes) {
            if (!runs.empty() && runs.back().off + runs.back().bytes == d.off) runs.back().bytes += d.bytes;
            else runs.push_back({ d.off, d.bytes });
        }
        end = d.off + d.bytes;
    }
    if (pl.total != end) return bad("total", which);
    if (pl.zero_bytes != zero_end) return bad("zero range", which);
    if ((size_t)pl.n_poison != runs.size()) return bad("number of poison ranges", which);
    for (size_t i = 0; i < runs.size(); ++i)
        if (pl.poison[i].off != runs[i].off || pl.poison[i].bytes != runs[i].bytes) return bad("poison range", which);
    return 0;
}

struct GeneralSizes {
    int n_cams = 0;
    size_t n_obs = 0, n_slots = 0, RB = 0, PF = 0, g_len = 0, part_rows = 0;
    bool merged = false, schurq = false;
    size_t sorted[1 + CCAL_MAX_CAMS] = {};
    GeneralLayout layout() const { return GeneralLayout(n_cams, n_obs, n_slots, RB, PF, g_len, part_rows, merged, schurq, sorted); }
};
static GeneralSizes rig_sizes(int n_cams, size_t n_slots, size_t n_obs, bool schurq, bool merged, bool with_sorted) {
    GeneralSizes z;
    const int K = 6 * n_cams + 6 * (n_cams - 1);                   // EUCM cameras
    z.n_cams = n_cams; z.n_obs = n_obs; z.n_slots = n_slots; z.RB = (size_t)red_size(K); z.PF = (size_t)pf_size(K);
    z.schurq = schurq; z.merged = merged;
    const size_t rs = (size_t)gen_rec_size(6);
    z.g_len = schurq ? 2 * std::max<size_t>(n_slots, 1) * rs : n_obs * rs;
    const size_t n_pw = (std::min<size_t>(std::max<size_t>(n_slots, 1), 4096) + 3) / 4 * 4;
    z.part_rows = std::max<size_t>(n_pw, schurq ? (std::max<size_t>(n_slots, 1) + 7) / 8 : n_pw / 4);
    if (with_sorted) {
        if (merged) z.sorted[0] = n_obs;
        else for (int c = 0; c < n_cams; ++c) z.sorted[1 + c] = n_obs / (size_t)n_cams + (c == 0 ? n_obs % (size_t)n_cams : 0);
    }
    return z;
}
static int check_general(const GeneralSizes& z) {
    const GeneralLayout l = z.layout();
    const size_t no = std::max<size_t>(z.n_obs, 1), ns = std::max<size_t>(z.n_slots, 1);
    const unsigned CD = kCleared | kDoubles;
    std::vector<Decl> d = {
        decl(l.G[0], std::max<size_t>(z.g_len, 1), CD), decl(l.G[1], std::max<size_t>(z.g_len, 1), CD), decl(l.cost_o[0], no, CD), decl(l.cost_o[1], no, CD),
        decl(l.partial, z.RB * z.part_rows, CD), decl(l.mc_slot, ns, CD), decl(l.scal, 8, CD), decl(l.flags, 4, kCleared),
        decl(l.red, 2 * (z.RB + 8), kDoubles), decl(l.pf, ns * z.PF, kDoubles), decl(l.gstate, 1),
        decl(l.goff, no), decl(l.slot_off, z.n_slots + 1), decl(l.slot_obs, no), decl(l.obs_cam, no), decl(l.caminfo, (size_t)z.n_cams * 4),
        decl(l.slot_desc, no), decl(l.obs_owner, no), decl(l.all_obs, z.merged ? no : 0), decl(l.slot_rec, z.schurq ? ns * 2 : 0) };
    for (int i = 0; i <= CCAL_MAX_CAMS; ++i) d.push_back(decl(l.sorted[i], z.sorted[i]));
    if (check("general workspace, device block", l.dev, d)) return 1;
    if (l.dev.n_poison != 2 || l.dev.poison[0].off != 0 || l.dev.poison[0].bytes != l.flags.off || l.dev.poison[1].off != l.red.off ||
        l.dev.poison[1].bytes != l.gstate.off - l.red.off) return bad("the poison touches G .. scal and red, pf - never flags, the state or a table", "general workspace");
    return check("general workspace, pinned block", l.host, { decl(l.h_gstatus, 1, kCleared), decl(l.h_gstate, 1), decl(l.h_pinned, z.RB + 16, kDoubles) });
}

static int checks() {
    for (int n_cams : { 2, 3, 5, 8 })
        for (int schurq = 0; schurq < (n_cams == 2 ? 2 : 1); ++schurq)
            for (int merged = 0; merged < 2; ++merged)
                for (int with_sorted = 0; with_sorted < 2; ++with_sorted)
                    for (size_t n_slots : { (size_t)0, (size_t)1, (size_t)37, (size_t)1200, (size_t)2500 }) {
                        const size_t n_obs = n_slots * (size_t)n_cams - n_slots / 7;
                        if (check_general(rig_sizes(n_cams, n_slots, n_obs, schurq != 0, merged != 0, with_sorted != 0 && n_obs >= 2000))) return 1;
                        if (check_general(rig_sizes(n_cams, n_slots, 0, schurq != 0, merged != 0, false))) return 1;          // n_obs = 0
                    }
    {
        const NormalBaseLayout l;
        if (check("dc | cols", l.plan, { decl(l.dc, CCAL_KMAX, kDoubles), decl(l.cols, CCAL_KMAX) })) return 1;
    }
    for (size_t n_obs : { (size_t)0, (size_t)1, (size_t)63, (size_t)600, (size_t)20000 }) {
        const PoseScratch l(n_obs);
        const size_t no = std::max<size_t>(n_obs, 1);
        if (check("scratch of ccal_init_poses", l.plan, { decl(l.poses, no * 6, kDoubles), decl(l.counts, no) })) return 1;
    }
    for (size_t n_off : { (size_t)0, (size_t)2, (size_t)601 })
        for (int64_t n : { (int64_t)1, (int64_t)31, (int64_t)8192, (int64_t)86400 }) {
            const StatsScratch l(n_off, n);
            if (check("scratch of validation()", l.plan, { decl(l.offsets, n_off), decl(l.values, (size_t)n, kDoubles), decl(l.work, kSelWorkBytes) })) return 1;
        }
    // order_stats_block_bytes: the values' room + the work area's (sizeof(SelWork) = 103 664)
    for (int64_t n : { (int64_t)1, (int64_t)8192, (int64_t)8193, (int64_t)1440000 })
        if (order_stats_block_bytes(n, nullptr) != ((size_t)n * 8 + 255) / 256 * 256 + (103664 + 255) / 256 * 256) return bad("order_stats_block_bytes", "scratch");
    if (order_stats_block_bytes(0, nullptr) != 0) return bad("order_stats_block_bytes(0)", "scratch");
    std::printf("LAYOUT-OK\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "golden")) return golden();
    if (argc == 2 && !std::strcmp(argv[1], "check")) return checks();
    if (argc == 4 && !std::strcmp(argv[1], "general")) {            // a two-camera EUCM rig under k_schurq (1 000 .. 8 192 slots): n_slots, n_obs
        const GeneralSizes z = rig_sizes(2, std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10), true, true, false);
        std::printf("general block %zu bytes\n", z.layout().dev.total);
        return 0;
    }
    return bad("usage: golden | check", "arguments");
}

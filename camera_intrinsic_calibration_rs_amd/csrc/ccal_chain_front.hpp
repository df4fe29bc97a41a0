// What the calls that start from images share on the host: the detector's slices of a call's block with the DetectArgs over them
// (ccal_detect_corners_* too), and the front of both chains (ccal_detect_tags_*, ccal_detect_checkerboards_*) - the options they
// begin with and their check, the refinement's slices and CornerArgs, and a chunk's way from images to refined candidates.  Host
// only, inline, no translation unit of its own; the kernels are the stages' (ccal_internal.hpp).
#pragma once
#include <algorithm>
#include <vector>
#include "ccal_call.hpp"
#include "ccal_tagchain_plan.hpp"

namespace ccal {

struct DetectSlices {
    Slice<char> img; Slice<int32_t> pix; Slice<long long> rmax; Slice<int32_t> hess; Slice<int64_t> resp; Slice<int32_t> rowoff, count;
    Slice<int64_t> imgoff; Slice<int32_t> oxy, ohess; Slice<int64_t> oresp;
    // images (host call) | slots | rows, counts, offsets | the stored rows, at most `rows` per image; nc images per chunk
    void add(CallBlock& blk, const GreyBatch& b, const DetectDomain& dm, size_t rows, size_t nc) {
        img = blk.add<char>(b.staged_bytes(nc)); pix = blk.add<int32_t>(dm.slots() * nc); rmax = blk.add<long long>(nc);
        hess = blk.add<int32_t>(3 * dm.slots() * nc); resp = blk.add<int64_t>(dm.slots() * nc);
        rowoff = blk.add<int32_t>((size_t)dm.dh * nc); count = blk.add<int32_t>(nc); imgoff = blk.add<int64_t>(nc + 1);
        oxy = blk.add<int32_t>(2 * rows * nc); ohess = blk.add<int32_t>(3 * rows * nc); oresp = blk.add<int64_t>(rows * nc);
    }
    // everything but img and n, which are a chunk's
    DetectArgs args(const CallBlock& blk, const GreyBatch& b, const DetectDomain& dm, int step, int nms_radius, int64_t min_response,
                    int rel_q10, int cap) const {
        DetectArgs da = {};
        da.W = b.width; da.H = b.height; da.s = step; da.r = nms_radius; da.rel_q10 = rel_q10; da.cap = cap; da.min_response = min_response;
        da.d0 = dm.d0; da.dw = dm.dw; da.dh = dm.dh; da.nbx = dm.nbx; da.nby = dm.nby;
        da.pix = blk.at(pix); da.hess = blk.at(hess); da.resp = blk.at(resp); da.rmax = blk.at(rmax);
        da.rowoff = blk.at(rowoff); da.count = blk.at(count); da.imgoff = blk.at(imgoff);
        da.oxy = blk.at(oxy); da.ohess = blk.at(ohess); da.oresp = blk.at(oresp);
        return da;
    }
};

struct FrontParams {               // the detector's and the refinement's options, with which both chains' options structs begin
    int32_t step, nms_radius; int64_t min_response; int32_t rel_q10, cand_cap, half_win, max_iterations; double eps;
    template <class Opts> static FrontParams of(const Opts& o) {
        return { o.step, o.nms_radius, o.min_response, o.rel_q10, o.cand_cap, o.half_win, o.max_iterations, o.eps };
    }
};
// the message of the first range missed (the ceiling's is written into buf), or nullptr: detector, the chain's ceiling on cand_cap, refinement
inline const char* front_bad_params(const FrontParams& p, int32_t cand_ceiling, char (&buf)[40]) {
    if (const char* what = detect_bad_params(p.step, p.nms_radius, p.min_response, p.rel_q10, p.cand_cap)) return what;
    if (p.cand_cap > cand_ceiling) { snprintf(buf, sizeof buf, "cand_cap outside 1 .. %d", (int)cand_ceiling); return buf; }
    return corners_bad_params(p.half_win, p.max_iterations, p.eps);
}

inline size_t clamped_total(const std::vector<int32_t>& v, size_t m, size_t cap) {      // a chunk's sum of a count the device reported, each within 0 .. cap
    size_t t = 0;
    for (size_t i = 0; i < m; ++i) t += std::min((size_t)std::max(v[i], 0), cap);
    return t;
}

// A chain adds its slices as front ints | its own ints | front doubles | its own doubles: the doubles the kernels write before they
// read lie together from `xy` on, so one poison(front.xy, <the chain's last double>) per chunk covers them.
struct ChainFront {
    DetectSlices det;
    Slice<int32_t> status, iters; Slice<double> xy, lam;
    DetectArgs da; CornerArgs ca;
    size_t cand = 0, nc = 0;       // stored rows per image, images per chunk
    void add_ints(CallBlock& blk, const GreyBatch& b, const DetectDomain& dm, size_t cand_rows, size_t per_chunk) {
        cand = cand_rows; nc = per_chunk;
        det.add(blk, b, dm, cand, nc);
        status = blk.add<int32_t>(cand * nc); iters = blk.add<int32_t>(cand * nc);
    }
    void add_doubles(CallBlock& blk) { xy = blk.add<double>(2 * cand * nc); lam = blk.add<double>(cand * nc); }
    void bind(const CallBlock& blk, const GreyBatch& b, const DetectDomain& dm, const FrontParams& p) {      // after blk.alloc()
        da = det.args(blk, b, dm, p.step, p.nms_radius, p.min_response, p.rel_q10, p.cand_cap);
        ca = {};
        ca.off = da.imgoff; ca.xy = blk.at(xy); ca.status = blk.at(status); ca.iters = blk.at(iters); ca.lam = blk.at(lam);
        ca.W = b.width; ca.H = b.height; ca.h = p.half_win; ca.max_it = p.max_iterations; ca.eps = p.eps;
    }
    // Steps 1 - 3 of both rules for the images k0 .. k0 + m - 1: candidates, offsets, stored rows; the host learns the counts (h_count:
    // room for nc); starts and refinement, enqueued only.  Returns the candidates stored, 0 also after a failure (blk.ok() tells).
    size_t run(CallBlock& blk, hipStream_t st, const GreyBatch& b, size_t k0, size_t m, std::vector<int32_t>& h_count) {
        da.n = ca.n_img = (int32_t)m;
        da.img = ca.img = b.chunk(blk, det.img, k0, m);
        if (blk.ok()) blk.note(detect_enqueue_find(st, b.dtype, da));
        if (blk.ok()) blk.note(tagchain_enqueue_offsets(st, da.count, cand, m, blk.at(det.imgoff)));
        if (blk.ok()) blk.note(detect_enqueue_emit(st, da));
        blk.download(h_count.data(), da.count, m);
        if (blk.ok()) blk.note(hipStreamSynchronize(st));
        if (!blk.ok()) return 0;
        const size_t n_cand = clamped_total(h_count, m, cand);
        if (!n_cand) return 0;
        ca.n = (int64_t)n_cand;
        blk.note(tagchain_enqueue_starts(st, da.oxy, ca.xy, (int64_t)(2 * n_cand)));
        if (blk.ok()) blk.note(corners_enqueue(st, b.dtype, ca));
        return n_cand;
    }
};

}  // namespace ccal

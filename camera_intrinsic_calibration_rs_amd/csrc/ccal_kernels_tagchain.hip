// From images to named tags in one call (ccal_detect_tags_batch / _dev): the four stages - detector, refinement, proposer, decoder -
// chained on the device by the rule stated at the entry points in include/ccal.h.  The stages' kernels are the ones their own entry
// points launch (ccal_internal.hpp), detector and refinement through the front shared with the board chain (ccal_chain_front.hpp); the links:
//   k_chain_starts     the detector's stored int32 rows to the refinement's f64 starts, same compact layout
//   k_chain_merge      one wavefront per image: the corners with status CCAL_OK, in candidate order, each rounded through f32 and tested
//                      against the points kept so far - the lanes stride the kept list, one __any decides.  The greedy order is
//                      sequential by definition; a block of 64 candidates is loaded at once and handed round by shuffles.  The first
//                      kMergeLds kept points live in LDS as the f32 pairs they are, the rest is read back from the output.
//   k_chain_compact    the kept points of every image moved to the compact layout the proposer indexes
//   k_chain_offsets    offsets[k + 1] = sum over i <= k of min(count[i], cap): one wavefront, a shuffle scan per 64 images
//   k_chain_quad_scan  one wavefront per image: base[] = the exclusive scan of the points' quad counts, the image's count, its cut bit
//   k_chain_select     one wavefront per image: a CCAL_TAG_OK quad keeps its id if no other OK quad of that id beats it under
//                      (hamming, -margin, row); its output row is the number of winners of a smaller id.  O(q^2 / 64) per image.
// Per chunk the host reads back per-image scalars only - candidate counts, kept points, quad counts and cut bits - to size the next
// stage's grid; no per-point or per-quad array leaves the device before the tags.  Every loop whose bound was read from device memory
// is clamped to the cap its arrays were sized with.  No atomics (the detector's integer max apart); every order is an index order.
// Comparisons and conversions only: no sum or product whose rounding a yardstick would have to follow.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "ccal_chain_front.hpp"
#include "ccal_image_device.hpp"

namespace ccal {

constexpr int kMergeLds = 2048;               // kept points held in LDS: 16 KB

__global__ __launch_bounds__(256) void k_chain_starts(const int32_t* __restrict__ in, double* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (double)in[i];
}

__global__ __launch_bounds__(64) void k_chain_offsets(const int32_t* __restrict__ count, int32_t cap, int32_t n, int64_t* __restrict__ off) {
    const int lane = threadIdx.x;
    int64_t carry = 0;
    if (lane == 0) off[0] = 0;
    for (int b0 = 0; b0 < n; b0 += 64) {
        const int i = b0 + lane;
        const int32_t c = i < n ? min(max(count[i], 0), cap) : 0;
        const int32_t inc = wave_scan_inclusive(c, lane);
        if (i < n) off[i + 1] = carry + inc;
        carry += __shfl(inc, 63, 64);
    }
}

__global__ __launch_bounds__(64) void k_chain_merge(const MergeArgs a) {
    __shared__ float kx[kMergeLds], ky[kMergeLds];
    const int k = blockIdx.x, lane = threadIdx.x;
    const int64_t first = a.off[k];
    const int m = csr_span(a.off, k, a.cap);
    double* out = a.out + 2 * first;
    int nk = 0;
    for (int b0 = 0; b0 < m; b0 += 64) {
        const int i = b0 + lane;
        bool live = false;
        float fx = 0.f, fy = 0.f;
        if (i < m) {
            live = !a.status || a.status[first + i] == CCAL_OK;
            fx = (float)a.xy[2 * (first + i)]; fy = (float)a.xy[2 * (first + i) + 1];      // round to nearest even
        }
        unsigned long long todo = __ballot(live);
        while (todo) {                                   // wave-uniform: the block's live candidates in index order
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const float cx = __shfl(fx, l, 64), cy = __shfl(fy, l, 64);
            const double px = (double)cx, py = (double)cy;
            bool hit = false;
            for (int j = lane; j < nk; j += 64) {
                const double qx = j < kMergeLds ? (double)kx[j] : out[2 * j], qy = j < kMergeLds ? (double)ky[j] : out[2 * j + 1];
                hit = hit || (fabs(qx - px) <= a.radius && fabs(qy - py) <= a.radius);     // exact differences of f32 values
            }
            if (!__any(hit)) {
                if (lane == 0) {
                    out[2 * nk] = px; out[2 * nk + 1] = py;
                    if (nk < kMergeLds) { kx[nk] = cx; ky[nk] = cy; }
                }
                ++nk;
                wave_handoff();                       // the next candidate's test reads this point
            }
        }
    }
    if (lane == 0) a.kept[k] = nk;
}

// grid (ceil(cap / 256), images): point j of image k from its place among the candidates to its place among the points
__global__ __launch_bounds__(256) void k_chain_compact(const int64_t* __restrict__ src_off, const int64_t* __restrict__ dst_off,
                                                       const double* __restrict__ src, double* __restrict__ dst, int32_t cap) {
    const int k = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= csr_span(dst_off, k, cap)) return;
    const int64_t s = src_off[k] + j, d = dst_off[k] + j;
    dst[2 * d] = src[2 * s]; dst[2 * d + 1] = src[2 * s + 1];
}

__global__ __launch_bounds__(64) void k_chain_quad_scan(const int64_t* __restrict__ off, const int32_t* __restrict__ deg,
                                                        const int32_t* __restrict__ cnt, int32_t* __restrict__ base,
                                                        int32_t* __restrict__ qcount, int32_t* __restrict__ qflags, int32_t cap) {
    const int k = blockIdx.x, lane = threadIdx.x;
    const int64_t first = off[k];
    const int m = csr_span(off, k, cap);
    int32_t carry = 0;                                   // at most 32768 * 8^3 = 2^24
    bool cut = false;
    for (int b0 = 0; b0 < m; b0 += 64) {
        const int i = b0 + lane;
        const int32_t c = i < m ? cnt[first + i] : 0;
        cut = cut || (i < m && deg[first + i] > CCAL_QUAD_MAX_OUT_EDGES);
        const int32_t inc = wave_scan_inclusive(c, lane);
        if (i < m) base[first + i] = carry + inc - c;
        carry += __shfl(inc, 63, 64);
    }
    const bool any_cut = __any(cut);
    if (lane == 0) { qcount[k] = carry; qflags[k] = any_cut ? 1 : 0; }
}

__global__ __launch_bounds__(64) void k_chain_select(const SelectArgs a) {
    const int k = blockIdx.x, lane = threadIdx.x;
    const int64_t first = a.off[k];
    const int q = csr_span(a.off, k, a.cap);
    const int32_t* reason = a.reason + first; const int32_t* id = a.id + first; const int32_t* ham = a.hamming + first;
    const double* margin = a.margin + first;
    int32_t* win = a.win + first;
    int n_ok = 0;
    for (int i0 = 0; i0 < q; i0 += 64) {
        const int i = i0 + lane;
        const bool ok = i < q && reason[i] == CCAL_TAG_OK;
        const int32_t my_id = ok ? id[i] : -1, my_ham = ok ? ham[i] : 0;
        const double my_margin = ok ? margin[i] : 0.0;
        bool beaten = false;
        for (int j = 0; j < q; ++j) {                    // wave-uniform
            if (reason[j] != CCAL_TAG_OK) continue;
            const int32_t hj = ham[j];
            const double mj = margin[j];
            const bool better = hj < my_ham || (hj == my_ham && (mj > my_margin || (mj == my_margin && j < i)));
            beaten = beaten || (ok && j != i && id[j] == my_id && better);
        }
        if (i < q) win[i] = ok && !beaten ? 1 : 0;
        n_ok += __popcll(__ballot(ok));
    }
    wave_handoff();
    int count = 0;
    for (int i0 = 0; i0 < q; i0 += 64) {
        const int i = i0 + lane;
        const bool mine = i < q && win[i] != 0;
        const int32_t my_id = mine ? id[i] : 0;
        int row = 0;
        for (int j = 0; j < q; ++j) row += (win[j] != 0 && id[j] < my_id) ? 1 : 0;
        if (mine && row < a.rows) {
            const int64_t o = (int64_t)k * a.rows + row;
            a.oid[o] = my_id; a.orot[o] = a.rot[first + i]; a.oham[o] = ham[i];
            a.omargin[o] = margin[i];
            for (int c = 0; c < 8; ++c) a.ocorners[8 * o + c] = a.corners[8 * (first + i) + c];
        }
        count += __popcll(__ballot(mine));
    }
    if (lane == 0) { a.count[k] = count; a.n_ok[k] = n_ok; }
}

hipError_t tagchain_enqueue_merge(hipStream_t s, const MergeArgs& a) {
    hipLaunchKernelGGL(k_chain_merge, dim3((unsigned)a.n_img), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t tagchain_enqueue_select(hipStream_t s, const SelectArgs& a) {
    hipLaunchKernelGGL(k_chain_select, dim3((unsigned)a.n_img), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t tagchain_enqueue_offsets(hipStream_t s, const int32_t* count, size_t cap, size_t n, int64_t* off) {
    hipLaunchKernelGGL(k_chain_offsets, dim3(1), dim3(64), 0, s, count, (int32_t)cap, (int32_t)n, off);
    return hipGetLastError();
}

hipError_t tagchain_enqueue_starts(hipStream_t s, const int32_t* in, double* out, int64_t n) {
    hipLaunchKernelGGL(k_chain_starts, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, n);
    return hipGetLastError();
}

namespace {

struct ChainOut {
    int32_t* count; int32_t* id; int32_t* rot; int32_t* hamming; double* corners; double* margin; int32_t* flags; int32_t* stats;
};

int tagchain_call(ccal_ctx* ctx, const char* where, const GreyBatch& b, int d, const uint64_t* codes, int n_codes,
                  const ccal_detect_tags_opts* o, const ChainOut& out) {
    const BadArg bad{ ctx, where };
    char buf[40];
    if (!o) return bad("NULL options");
    const FrontParams fp = FrontParams::of(*o);
    if (const char* what = front_bad_params(fp, (int32_t)kQuadMaxPoints, buf)) return bad(what);
    if (!(o->merge_radius >= 0.0) || !std::isfinite(o->merge_radius)) return bad("merge_radius negative or not finite");
    if (const char* what = quads_bad_params(o->min_side, o->max_side, o->max_side_ratio, o->offset, o->edge_samples, o->edge_min_contrast,
                                            o->quad_cap)) return bad(what);
    if (const char* what = tags_bad_params(d, o->border, n_codes, o->cell_samples, o->tag_min_contrast, o->max_border_errors, o->max_hamming))
        return bad(what);
    if (o->tag_cap < 1) return bad("tag_cap < 1");
    if (const char* what = b.bad()) return bad(what);
    if (const char* what = tags_bad_codes(d, codes, n_codes)) return bad(what);
    if (b.n_img == 0) return CCAL_OK;
    if (!b.images || !codes || !out.count || !out.id || !out.rot || !out.hamming || !out.corners || !out.flags) return bad("NULL argument");

    const int dtype = b.dtype, width = b.width, height = b.height;
    const size_t ni = (size_t)b.n_img, tag_cap = (size_t)o->tag_cap;
    std::fill(out.count, out.count + ni, 0);
    std::fill(out.flags, out.flags + ni, 0);
    if (out.stats) std::fill(out.stats, out.stats + 4 * ni, 0);
    const ChainShape sh = chain_shape((size_t)width, (size_t)height, dtype == CCAL_PIX_U16 ? 2 : 1, (size_t)o->step, (size_t)o->nms_radius,
                                      (size_t)o->cand_cap, (size_t)o->quad_cap, tag_cap, (size_t)n_codes);
    if (!sh.slots) return CCAL_OK;                        // no domain: nothing to launch
    const size_t C = sh.cand, Q = sh.quads, T = sh.tags;
    const size_t nc = chain_images_per_chunk(ni, chain_per_image_bytes(b.on_device, sh),
                                             test_chunk_bytes("CCAL_TEST_TAGCHAIN_CHUNK_BYTES", kChainChunkBytes));

    // one block for the largest chunk.  The doubles the kernels write before they read lie together: one poison covers them.
    CallBlock blk(ctx);
    const auto s_codes = blk.add<unsigned long long>((size_t)n_codes);
    ChainFront front;
    front.add_ints(blk, b, sh.dom, C, nc);
    const auto s_kept = blk.add<int32_t>(nc);
    const auto s_ptoff = blk.add<int64_t>(nc + 1);
    const auto s_adj = blk.add<int32_t>(CCAL_QUAD_MAX_OUT_EDGES * C * nc);
    const auto s_deg = blk.add<int32_t>(C * nc);
    const auto s_cnt = blk.add<int32_t>(C * nc);
    const auto s_base = blk.add<int32_t>(C * nc);
    const auto s_qcount = blk.add<int32_t>(nc);
    const auto s_qflags = blk.add<int32_t>(nc);
    const auto s_quadoff = blk.add<int64_t>(nc + 1);
    const auto s_oidx = blk.add<int32_t>(4 * Q * nc);
    const auto s_reason = blk.add<int32_t>(Q * nc);
    const auto s_id = blk.add<int32_t>(Q * nc);
    const auto s_rot = blk.add<int32_t>(Q * nc);
    const auto s_ham = blk.add<int32_t>(Q * nc);
    const auto s_code = blk.add<unsigned long long>(Q * nc);
    const auto s_win = blk.add<int32_t>(Q * nc);
    const auto s_ntags = blk.add<int32_t>(nc);
    const auto s_nok = blk.add<int32_t>(nc);
    const auto s_tid = blk.add<int32_t>(T * nc);
    const auto s_trot = blk.add<int32_t>(T * nc);
    const auto s_tham = blk.add<int32_t>(T * nc);
    front.add_doubles(blk);                               // the doubles, from here on
    const auto s_mxy = blk.add<double>(2 * C * nc);
    const auto s_pxy = blk.add<double>(2 * C * nc);
    const auto s_oquads = blk.add<double>(8 * Q * nc);
    const auto s_corners = blk.add<double>(8 * Q * nc);
    const auto s_margin = blk.add<double>(Q * nc);
    const auto s_tcorners = blk.add<double>(8 * T * nc);
    const auto s_tmargin = blk.add<double>(T * nc);
    if (!blk.alloc()) return blk.finish(where);

    front.bind(blk, b, sh.dom, fp);
    MergeArgs ma = {};
    ma.off = front.ca.off; ma.xy = front.ca.xy; ma.status = front.ca.status; ma.out = blk.at(s_mxy); ma.kept = blk.at(s_kept);
    ma.cap = (int32_t)C; ma.radius = o->merge_radius;
    QuadArgs qa = {};
    qa.off = blk.at(s_ptoff); qa.xy = blk.at(s_pxy); qa.adj = blk.at(s_adj); qa.deg = blk.at(s_deg); qa.cnt = blk.at(s_cnt);
    qa.base = blk.at(s_base); qa.rowoff = blk.at(s_quadoff); qa.oidx = blk.at(s_oidx); qa.oquads = blk.at(s_oquads);
    qa.p0 = 0; qa.W = width; qa.H = height;
    quads_set_params(qa, o->min_side, o->max_side, o->max_side_ratio, o->offset, o->edge_samples, o->edge_min_contrast, o->quad_cap);
    TagArgs ta = {};
    ta.off = blk.at(s_quadoff); ta.quads = blk.at(s_oquads); ta.codes = blk.at(s_codes);
    ta.reason = blk.at(s_reason); ta.id = blk.at(s_id); ta.rot = blk.at(s_rot); ta.hamming = blk.at(s_ham);
    ta.corners = blk.at(s_corners); ta.code = blk.at(s_code); ta.margin = blk.at(s_margin);
    ta.q0 = 0; ta.W = width; ta.H = height; ta.d = d; ta.border = o->border; ta.n_codes = n_codes; ta.S = o->cell_samples;
    ta.max_border = o->max_border_errors; ta.max_hamming = o->max_hamming; ta.min_contrast = o->tag_min_contrast;
    SelectArgs sa = {};
    sa.off = blk.at(s_quadoff); sa.reason = ta.reason; sa.id = ta.id; sa.rot = ta.rot; sa.hamming = ta.hamming;
    sa.corners = ta.corners; sa.margin = ta.margin; sa.win = blk.at(s_win); sa.count = blk.at(s_ntags); sa.n_ok = blk.at(s_nok);
    sa.oid = blk.at(s_tid); sa.orot = blk.at(s_trot); sa.oham = blk.at(s_tham); sa.ocorners = blk.at(s_tcorners); sa.omargin = blk.at(s_tmargin);
    sa.cap = (int32_t)Q; sa.rows = (int32_t)T;
    blk.upload(s_codes, codes, (size_t)n_codes);

    hipStream_t st = ctx->stream;
    std::vector<int32_t> h_count(nc), h_kept(nc), h_qcount(nc), h_qflags(nc), h_ntags(nc), h_nok(nc), h_id(T * nc), h_rot(T * nc), h_ham(T * nc);
    std::vector<double> h_corners(8 * T * nc), h_margin(out.margin ? T * nc : 0);

    for (size_t k0 = 0; k0 < ni && blk.ok(); k0 += nc) {
        const size_t m = std::min(nc, ni - k0);
        ma.n_img = qa.n_img = ta.n_img = sa.n_img = (int32_t)m;
        blk.poison(front.xy, s_tmargin);                  // the test hook's NaN over the doubles the kernels write before they read
        for (auto* v : { &h_kept, &h_qcount, &h_qflags, &h_ntags, &h_nok }) std::fill(v->begin(), v->end(), 0);     // a stage that does not run leaves zeros

        // 1. - 3. candidates, their offsets and stored rows; the host learns the counts; starts and refinement
        const size_t n_cand = front.run(blk, st, b, k0, m, h_count);
        if (!blk.ok()) break;
        qa.img = ta.img = front.da.img;

        // 4. - 5. rounding and merge, the points' compact layout; the host learns the kept counts
        if (n_cand) {
            blk.note(tagchain_enqueue_merge(st, ma));
            if (blk.ok()) blk.note(tagchain_enqueue_offsets(st, ma.kept, C, m, blk.at(s_ptoff)));
            if (blk.ok()) {
                hipLaunchKernelGGL(k_chain_compact, dim3((unsigned)((C + 255) / 256), (unsigned)m), dim3(256), 0, st, ma.off, blk.at(s_ptoff),
                                   ma.out, blk.at(s_pxy), (int32_t)C);
                blk.launched();
            }
            blk.download(h_kept.data(), ma.kept, m);
            if (blk.ok()) blk.note(hipStreamSynchronize(st));
            if (!blk.ok()) break;
        }
        const size_t n_pts = clamped_total(h_kept, m, C);

        // 6. edges and the count walk, the two scans; the host learns the quad counts and cut bits
        if (n_pts) {
            qa.n = (int64_t)n_pts;
            blk.note(quads_enqueue_count(st, dtype, qa));
            if (blk.ok()) {
                hipLaunchKernelGGL(k_chain_quad_scan, dim3((unsigned)m), dim3(64), 0, st, qa.off, qa.deg, qa.cnt, blk.at(s_base), blk.at(s_qcount),
                                   blk.at(s_qflags), (int32_t)C);
                blk.launched();
            }
            if (blk.ok()) blk.note(tagchain_enqueue_offsets(st, blk.at(s_qcount), Q, m, blk.at(s_quadoff)));
            blk.download(h_qcount.data(), blk.at(s_qcount), m);
            blk.download(h_qflags.data(), blk.at(s_qflags), m);
            if (blk.ok()) blk.note(hipStreamSynchronize(st));
            if (!blk.ok()) break;
        }
        const size_t n_quads = clamped_total(h_qcount, m, Q);

        // 6. - 8. the stored quads, the decoder, the selection; the tags come back
        if (n_quads) {
            ta.n = (int64_t)n_quads;
            blk.note(quads_enqueue_write(st, qa));
            if (blk.ok()) blk.note(tags_enqueue(st, dtype, ta));
            if (blk.ok()) blk.note(tagchain_enqueue_select(st, sa));
            blk.download(h_ntags.data(), sa.count, m);
            blk.download(h_nok.data(), sa.n_ok, m);
            blk.download(h_id.data(), sa.oid, T * m);
            blk.download(h_rot.data(), sa.orot, T * m);
            blk.download(h_ham.data(), sa.oham, T * m);
            blk.download(h_corners.data(), sa.ocorners, 8 * T * m);
            blk.download(out.margin ? h_margin.data() : nullptr, sa.omargin, T * m);
            if (blk.ok()) blk.note(hipStreamSynchronize(st));
            if (!blk.ok()) break;
        }

        for (size_t i = 0; i < m; ++i) {                   // to [k][tag_cap] of the caller's arrays
            const size_t k = k0 + i, rows = std::min((size_t)std::max(h_ntags[i], 0), T);
            out.count[k] = h_ntags[i];
            out.flags[k] = (h_qflags[i] & 1) | (h_count[i] > o->cand_cap ? 2 : 0) | (h_qcount[i] > o->quad_cap ? 4 : 0) |
                           ((size_t)std::max(h_ntags[i], 0) > tag_cap ? 8 : 0);
            if (out.stats) {
                out.stats[4 * k] = h_count[i]; out.stats[4 * k + 1] = h_kept[i]; out.stats[4 * k + 2] = h_qcount[i]; out.stats[4 * k + 3] = h_nok[i];
            }
            if (!rows) continue;
            std::memcpy(out.id + k * tag_cap, h_id.data() + i * T, rows * sizeof(int32_t));
            std::memcpy(out.rot + k * tag_cap, h_rot.data() + i * T, rows * sizeof(int32_t));
            std::memcpy(out.hamming + k * tag_cap, h_ham.data() + i * T, rows * sizeof(int32_t));
            std::memcpy(out.corners + 8 * k * tag_cap, h_corners.data() + 8 * i * T, rows * 8 * sizeof(double));
            if (out.margin) std::memcpy(out.margin + k * tag_cap, h_margin.data() + i * T, rows * sizeof(double));
        }
    }
    return blk.finish(where);
}

}  // namespace
}  // namespace ccal

using namespace ccal;

extern "C" {

int ccal_detect_tags_batch(ccal_ctx* ctx, int dtype, int width, int height, int n_img, const void* images, int d, const uint64_t* codes,
                           int n_codes, const ccal_detect_tags_opts* opts, int32_t* count_out, int32_t* id_out, int32_t* rot_out,
                           int32_t* hamming_out, double* corners_out, double* margin_out, int32_t* flags_out, int32_t* stats_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    return tagchain_call(ctx, "ccal_detect_tags_batch", GreyBatch{ dtype, width, height, n_img, images, false }, d, codes, n_codes, opts,
                         ChainOut{ count_out, id_out, rot_out, hamming_out, corners_out, margin_out, flags_out, stats_out });
    CCAL_API_CATCH(ctx)
}

int ccal_detect_tags_dev(ccal_ctx* ctx, int dtype, int width, int height, int n_img, const void* images_dev, int d, const uint64_t* codes,
                         int n_codes, const ccal_detect_tags_opts* opts, int32_t* count_out, int32_t* id_out, int32_t* rot_out,
                         int32_t* hamming_out, double* corners_out, double* margin_out, int32_t* flags_out, int32_t* stats_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    return tagchain_call(ctx, "ccal_detect_tags_dev", GreyBatch{ dtype, width, height, n_img, images_dev, true }, d, codes, n_codes, opts,
                         ChainOut{ count_out, id_out, rot_out, hamming_out, corners_out, margin_out, flags_out, stats_out });
    CCAL_API_CATCH(ctx)
}

}  // extern "C"

// Quad proposal (ccal_propose_quads_batch / _dev): the refined saddle points of a batch of grey images grouped into candidate tag
// outlines, by the rule stated at the entry points in include/ccal.h.  Per chunk of whole images three launches, one wavefront per
// point A, four per workgroup, no LDS, no barriers, no atomics:
//   edges    k_quad_edges: the lanes stride B over the points of A's image in blocks of 64; a lane runs the length test and then its
//            own 2 K bilinear f64 samples, and stops once bright - dark has fallen below the threshold (min and max are monotone: the
//            decision is the same).  The passing lanes of a block are one __ballot mask, a lane's slot is the running count plus the
//            popcount of the lower mask bits - index order; the first kQuadMaxOut go to adj[A][.], deg[A] keeps the full count.
//   count    k_quad_chains<false>: the at most 8^3 chains (i, j, k) over the three out-edge lists, 64 per pass in that order - i is
//            the pass, so wave-uniform; the lists are sorted, so this is the (B, C, D) index order.  cnt[A] = A's quads.
//   write    k_quad_chains<true>: the same walk, each quad to the row base[A] + its rank in the walk, below the cap.
// Between count and write the host reads deg and cnt (8 bytes per point), forms per image the count, the flags and the exclusive
// scan base[] - the point at which it has to synchronise anyway, to size the block of the stored rows - so no per-corner cap enters
// the rule and the rows of an image are in lexicographic order of (A, B, C, D) whatever the batch looks like.
// An image's outputs are a pure function of that image, its points and the parameters.  This unit is compiled with
// -ffp-contract=off (csrc/Makefile): the outputs are decisions, and tests/quad_ref.py, the numpy f64 yardstick, rounds every product
// and sum on its own.  Every pixel index is clamped to the image; the inside test makes the clamp a no-op, the clamp stays as the guard.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "ccal_call.hpp"
#include "ccal_image_device.hpp"
#include "ccal_image_plan.hpp"

namespace ccal {

constexpr int kQuadWaves = 4;                 // wavefronts (= points A in flight) per workgroup
constexpr int kQuadMaxOut = CCAL_QUAD_MAX_OUT_EDGES;
constexpr int kQuadMaxSamples = 16;
constexpr size_t kQuadChunkBytes = (size_t)256 << 20;     // the block one launch should need: larger batches go image chunk by chunk
static_assert(kQuadMaxOut == 8, "a pass of 64 lanes is one i and all (j, k)");

// QuadArgs: ccal_internal.hpp

// the point of wavefront g: its image k (the last with off[k] <= p0 + g; images without points are stepped over), the chunk
// index of the image's first point, the image's point count
__device__ __forceinline__ void quad_locate(const QuadArgs& a, int64_t g, int& k, int64_t& first, int& m) {
    k = image_of_row(a.off, a.n_img, a.p0 + g);
    first = a.off[k] - a.p0;
    m = (int)(a.off[k + 1] - a.off[k]);
}

template <class T>
__global__ __launch_bounds__(64 * kQuadWaves) void k_quad_edges(const QuadArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * kQuadWaves + wave;
    if (g >= a.n) return;                                // wave-uniform; the kernel has no barrier
    int k, m;
    int64_t first;
    quad_locate(a, g, k, first, m);
    const int la = (int)(g - first);
    const T* img = static_cast<const T*>(a.img) + (int64_t)k * a.W * a.H;
    const double* P = a.xy + 2 * first;
    const double Ax = P[2 * la], Ay = P[2 * la + 1];
    const double x_hi = (double)(a.W - 1), y_hi = (double)(a.H - 1), k1 = (double)(a.K + 1);
    int run = 0;
    for (int b0 = 0; b0 < m; b0 += 64) {
        const int b = b0 + lane;
        bool edge = false;
        if (b < m && b != la) {
            const double ex = P[2 * b] - Ax, ey = P[2 * b + 1] - Ay;
            const double L2 = ex * ex + ey * ey;
            if (L2 >= a.min2 && L2 <= a.max2) {          // false for NaN
                const double nx = -a.offset * ey, ny = a.offset * ex;
                double dark = -__builtin_inf(), bright = __builtin_inf();
                edge = true;
                for (int s = 0; s < a.K && edge; ++s) {
                    const double t = (double)(s + 1) / k1;
                    const double px = Ax + t * ex, py = Ay + t * ey;
                    const double xi = px + nx, yi = py + ny, xo = px - nx, yo = py - ny;
                    edge = xi >= 0.0 && xi <= x_hi && yi >= 0.0 && yi <= y_hi && xo >= 0.0 && xo <= x_hi && yo >= 0.0 && yo <= y_hi;
                    if (edge) {
                        dark = fmax(dark, image_sample(img, a.W, a.H, xi, yi));
                        bright = fmin(bright, image_sample(img, a.W, a.H, xo, yo));
                        edge = bright - dark >= a.min_contrast;      // it only falls from here on
                    }
                }
            }
        }
        const unsigned long long mask = __ballot(edge);
        if (edge) {
            const int slot = run + __popcll(mask & ((1ull << lane) - 1ull));
            if (slot < kQuadMaxOut) a.adj[(int64_t)kQuadMaxOut * g + slot] = b;
        }
        run += __popcll(mask);
    }
    if (lane == 0) a.deg[g] = run;
}

template <bool kWrite>
__global__ __launch_bounds__(64 * kQuadWaves) void k_quad_chains(const QuadArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * kQuadWaves + wave;
    if (g >= a.n) return;
    int img_k, m;
    int64_t first;
    quad_locate(a, g, img_k, first, m);
    const int A = (int)(g - first);
    const int32_t* adj = a.adj + kQuadMaxOut * first;    // the image's lists and degrees, by local index
    const int32_t* deg = a.deg + first;
    const double* P = a.xy + 2 * first;
    const int dA = min(deg[A], kQuadMaxOut);
    const double Ax = P[2 * A], Ay = P[2 * A + 1];
    int run = kWrite ? a.base[g] : 0;                    // quads of the image in front of the pass's first
    const int64_t row0 = kWrite ? a.rowoff[img_k] : 0;
    const int j = lane >> 3, kk = lane & 7;
    for (int i = 0; i < dA; ++i) {                       // pass i: the chains (i, j, kk), 64 in order of the lane number
        if (kWrite && run >= a.cap) break;
        const int B = adj[kQuadMaxOut * A + i];
        bool quad = false;
        int Cc = 0, D = 0;
        if (A < B && j < min(deg[B], kQuadMaxOut)) {
            Cc = adj[kQuadMaxOut * B + j];
            if (A < Cc && kk < min(deg[Cc], kQuadMaxOut)) {
                D = adj[kQuadMaxOut * Cc + kk];
                bool closes = false;
                if (A < D && D != B) {
                    const int dD = min(deg[D], kQuadMaxOut);
                    for (int t = 0; t < dD; ++t) closes = closes || adj[kQuadMaxOut * D + t] == A;
                }
                if (closes) {
                    const double e1x = P[2 * B] - Ax, e1y = P[2 * B + 1] - Ay;
                    const double e2x = P[2 * Cc] - P[2 * B], e2y = P[2 * Cc + 1] - P[2 * B + 1];
                    const double e3x = P[2 * D] - P[2 * Cc], e3y = P[2 * D + 1] - P[2 * Cc + 1];
                    const double e4x = Ax - P[2 * D], e4y = Ay - P[2 * D + 1];
                    const bool convex = e1x * e2y - e1y * e2x > 0.0 && e2x * e3y - e2y * e3x > 0.0 && e3x * e4y - e3y * e4x > 0.0 &&
                                        e4x * e1y - e4y * e1x > 0.0;
                    const double s1 = e1x * e1x + e1y * e1y, s2 = e2x * e2x + e2y * e2y, s3 = e3x * e3x + e3y * e3y, s4 = e4x * e4x + e4y * e4y;
                    const double smax = fmax(fmax(s1, s2), fmax(s3, s4)), smin = fmin(fmin(s1, s2), fmin(s3, s4));
                    quad = convex && smax <= a.ratio2 * smin;
                }
            }
        }
        const unsigned long long mask = __ballot(quad);
        if (kWrite && quad) {
            const int r = run + __popcll(mask & ((1ull << lane) - 1ull));
            if (r < a.cap) {
                const int64_t row = row0 + r;
                a.oidx[4 * row] = A; a.oidx[4 * row + 1] = B; a.oidx[4 * row + 2] = Cc; a.oidx[4 * row + 3] = D;
                if (a.oquads) {
                    double* q = a.oquads + 8 * row;
                    q[0] = Ax; q[1] = Ay; q[2] = P[2 * B]; q[3] = P[2 * B + 1];
                    q[4] = P[2 * Cc]; q[5] = P[2 * Cc + 1]; q[6] = P[2 * D]; q[7] = P[2 * D + 1];
                }
            }
        }
        run += __popcll(mask);
    }
    if (!kWrite && lane == 0) a.cnt[g] = run;
}

const char* quads_bad_params(double min_side, double max_side, double max_side_ratio, double offset, int samples, double min_contrast, int cap) {
    if (!(min_side >= 1.0)) return "min_side < 1";
    if (!(max_side >= min_side)) return "max_side < min_side";
    if (!(max_side_ratio >= 1.0)) return "max_side_ratio < 1";
    if (!(offset > 0.0 && offset <= 0.25)) return "offset outside (0, 0.25]";
    if (samples < 1 || samples > kQuadMaxSamples) return "samples outside 1 .. 16";
    if (!(min_contrast >= 0.0) || !std::isfinite(min_contrast)) return "min_contrast negative or not finite";
    if (cap < 1) return "cap < 1";
    return nullptr;
}

// the squares are formed here, in the unit without fused multiply-adds, for every caller alike
void quads_set_params(QuadArgs& a, double min_side, double max_side, double max_side_ratio, double offset, int samples, double min_contrast, int cap) {
    a.K = samples; a.cap = cap;
    a.min2 = min_side * min_side; a.max2 = max_side * max_side; a.ratio2 = max_side_ratio * max_side_ratio;
    a.offset = offset; a.min_contrast = min_contrast;
}

hipError_t quads_enqueue_count(hipStream_t s, int dtype, const QuadArgs& a) {
    const dim3 grid((unsigned)(((size_t)a.n + kQuadWaves - 1) / kQuadWaves)), block(64 * kQuadWaves);
    for_pix_type(dtype, [&](auto t) { hipLaunchKernelGGL(k_quad_edges<decltype(t)>, grid, block, 0, s, a); });
    hipLaunchKernelGGL(k_quad_chains<false>, grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t quads_enqueue_write(hipStream_t s, const QuadArgs& a) {
    const dim3 grid((unsigned)(((size_t)a.n + kQuadWaves - 1) / kQuadWaves)), block(64 * kQuadWaves);
    hipLaunchKernelGGL(k_quad_chains<true>, grid, block, 0, s, a);
    return hipGetLastError();
}

namespace {

int quads_call(ccal_ctx* ctx, const char* where, const GreyBatch& b, const int64_t* offsets, const double* xy, double min_side, double max_side,
               double max_side_ratio, double offset, int samples, double min_contrast, int cap, int32_t* count_out, int32_t* flags_out,
               int32_t* idx_out, double* quads_out) {
    const BadArg bad{ ctx, where };
    if (const char* what = quads_bad_params(min_side, max_side, max_side_ratio, offset, samples, min_contrast, cap)) return bad(what);
    if (const char* what = b.bad()) return bad(what);
    const int n_img = b.n_img;
    if (n_img == 0) return CCAL_OK;
    if (!b.images || !offsets || !count_out || !flags_out || !idx_out) return bad("NULL argument");
    if (check_offsets(ctx, where, "offsets", offsets, (size_t)n_img, 0)) return CCAL_ERR_INVALID_ARG;
    if (offsets[n_img] > (int64_t)INT32_MAX) return bad("more than 2^31 - 1 points");
    for (int k = 0; k < n_img; ++k)
        if (offsets[k + 1] - offsets[k] > kQuadMaxPoints) return bad("more than 32768 points in an image");
    if (offsets[n_img] > 0 && !xy) return bad("NULL argument");
    std::fill(count_out, count_out + n_img, 0);
    std::fill(flags_out, flags_out + n_img, 0);
    if (offsets[n_img] == 0) return CCAL_OK;

    // chunks of whole images: as many as keep the chunk's images (host call), points and work arrays within the limit, at least one
    static_assert(kQuadPerPointBytes == 2 * sizeof(double) + (kQuadMaxOut + 3) * sizeof(int32_t), "xy | adj | deg, cnt, base");
    const ImageChunks plan = image_chunks(offsets, (size_t)n_img, b.staged_bytes(1) + kQuadPerImageBytes, kQuadPerPointBytes,
                                          test_chunk_bytes("CCAL_TEST_QUADS_CHUNK_BYTES", kQuadChunkBytes));
    const std::vector<size_t>& cut = plan.cut;
    const size_t max_img = plan.max_img, max_pts = plan.max_rows;

    // one block for the largest chunk: offsets, row offsets | images (host call) | points | lists, degrees, counts, bases
    CallBlock blk(ctx);
    const auto s_off = blk.add<int64_t>(max_img + 1);
    const auto s_rowoff = blk.add<int64_t>(max_img + 1);
    const auto s_img = blk.add<char>(b.staged_bytes(max_img));
    const auto s_xy = blk.add<double>(2 * max_pts);
    const auto s_adj = blk.add<int32_t>(kQuadMaxOut * max_pts);
    const auto s_deg = blk.add<int32_t>(max_pts);
    const auto s_cnt = blk.add<int32_t>(max_pts);
    const auto s_base = blk.add<int32_t>(max_pts);
    if (!blk.alloc()) return blk.finish(where);

    QuadArgs a = {};
    a.off = blk.at(s_off); a.rowoff = blk.at(s_rowoff); a.xy = blk.at(s_xy);
    a.adj = blk.at(s_adj); a.deg = blk.at(s_deg); a.cnt = blk.at(s_cnt); a.base = blk.at(s_base);
    a.W = b.width; a.H = b.height;
    quads_set_params(a, min_side, max_side, max_side_ratio, offset, samples, min_contrast, cap);
    std::vector<int32_t> h_deg(max_pts), h_cnt(max_pts), h_base(max_pts), h_idx;
    std::vector<int64_t> rowoff(max_img + 1);
    std::vector<double> h_quads;

    for (size_t c = 0; c + 1 < cut.size() && blk.ok(); ++c) {
        const size_t k0 = cut[c], m = cut[c + 1] - k0;
        const size_t at = (size_t)offsets[k0], np = (size_t)(offsets[k0 + m] - offsets[k0]);
        if (!np) continue;
        a.n_img = (int32_t)m; a.p0 = offsets[k0]; a.n = (int64_t)np;
        blk.upload(s_off, offsets + k0, m + 1);
        a.img = b.chunk(blk, s_img, k0, m);
        blk.upload(s_xy, xy + 2 * at, 2 * np);
        if (blk.ok()) blk.note(quads_enqueue_count(ctx->stream, b.dtype, a));
        blk.download(h_deg.data(), a.deg, np);
        blk.download(h_cnt.data(), a.cnt, np);
        if (blk.ok()) blk.note(hipStreamSynchronize(ctx->stream));
        if (!blk.ok()) break;

        // per image: the count, the flags, the exclusive scan of the points' counts, the stored rows
        rowoff[0] = 0;
        for (size_t i = 0; i < m; ++i) {
            int64_t count = 0;
            int32_t flags = 0;
            for (size_t p = (size_t)offsets[k0 + i] - at, e = (size_t)offsets[k0 + i + 1] - at; p < e; ++p) {
                h_base[p] = (int32_t)count;               // at most 32768 * 8^3 = 2^24
                count += h_cnt[p];
                if (h_deg[p] > kQuadMaxOut) flags |= 1;
            }
            count_out[k0 + i] = (int32_t)count;
            flags_out[k0 + i] = flags;
            rowoff[i + 1] = rowoff[i] + std::min<int64_t>(count, (int64_t)cap);
        }
        const size_t total = (size_t)rowoff[m];
        if (!total) continue;

        // the stored rows of the chunk, image after image: a block of exactly their size
        CallBlock rows(ctx);
        const auto s_oidx = rows.add<int32_t>(4 * total);
        const auto s_oquads = rows.add<double>(quads_out ? 8 * total : 0);
        if (!rows.alloc()) return rows.finish(where);
        a.oidx = rows.at(s_oidx); a.oquads = rows.at(s_oquads);
        if (quads_out) rows.poison(s_oquads, s_oquads);   // the test hook's NaN over the doubles the kernel writes and never reads
        blk.upload(s_base, h_base.data(), np);
        blk.upload(s_rowoff, rowoff.data(), m + 1);
        if (!blk.ok()) break;                             // no launch: nothing of the unwritten rows reaches the caller's arrays
        if (rows.ok()) rows.note(quads_enqueue_write(ctx->stream, a));
        h_idx.resize(4 * total);
        if (quads_out) h_quads.resize(8 * total);
        rows.download(h_idx.data(), a.oidx, 4 * total);
        rows.download(quads_out ? h_quads.data() : nullptr, a.oquads, 8 * total);
        const int rc = rows.finish(where);                // synchronises
        if (rc != CCAL_OK) return rc;
        for (size_t i = 0; i < m; ++i) {                  // to [k][cap] of the caller's arrays
            const size_t r0 = (size_t)rowoff[i], nr = (size_t)(rowoff[i + 1] - rowoff[i]), k = k0 + i;
            if (!nr) continue;
            std::memcpy(idx_out + 4 * k * (size_t)cap, h_idx.data() + 4 * r0, nr * 4 * sizeof(int32_t));
            if (quads_out) std::memcpy(quads_out + 8 * k * (size_t)cap, h_quads.data() + 8 * r0, nr * 8 * sizeof(double));
        }
    }
    return blk.finish(where);
}

}  // namespace
}  // namespace ccal

using namespace ccal;

extern "C" {

int ccal_propose_quads_batch(ccal_ctx* ctx, int dtype, int width, int height, int n_img, const void* images, const int64_t* offsets,
                             const double* xy, double min_side, double max_side, double max_side_ratio, double offset, int samples,
                             double min_contrast, int cap, int32_t* count_out, int32_t* flags_out, int32_t* idx_out, double* quads_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    return quads_call(ctx, "ccal_propose_quads_batch", GreyBatch{ dtype, width, height, n_img, images, false }, offsets, xy, min_side,
                      max_side, max_side_ratio, offset, samples, min_contrast, cap, count_out, flags_out, idx_out, quads_out);
    CCAL_API_CATCH(ctx)
}

int ccal_propose_quads_dev(ccal_ctx* ctx, int dtype, int width, int height, int n_img, const void* images_dev, const int64_t* offsets,
                           const double* xy, double min_side, double max_side, double max_side_ratio, double offset, int samples,
                           double min_contrast, int cap, int32_t* count_out, int32_t* flags_out, int32_t* idx_out, double* quads_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    return quads_call(ctx, "ccal_propose_quads_dev", GreyBatch{ dtype, width, height, n_img, images_dev, true }, offsets, xy, min_side,
                      max_side, max_side_ratio, offset, samples, min_contrast, cap, count_out, flags_out, idx_out, quads_out);
    CCAL_API_CATCH(ctx)
}

}  // extern "C"

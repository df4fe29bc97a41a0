// Sub-pixel corner refinement (ccal_refine_corners_batch / _dev): every coarse corner of a batch of grey images moved onto the
// grey-level saddle by the gradient-orthogonality fit stated at the entry points in include/ccal.h.  All corners of all images in
// ONE launch, one wavefront per corner, four per workgroup, the whole iteration of a corner inside the launch:
//   patch    lanes stride the (2h+3)^2 positions around the iterate: four pixel loads and the f64 bilinear blend each, into the
//            wavefront's own LDS patch (row stride 2h+3: odd, so a lane group's f64 rows do not pile on one bank pair)
//   sums     lanes stride the (2h+1)^2 window: central differences out of the patch, the separable weight out of a 2h+1 table the
//            wavefront filled once, five lane-private f64 sums; one xor-shuffle butterfly leaves the same totals on all 64 lanes
//   decide   every lane: the 2 x 2 solve, the inside / degenerate / stop / drift rules - wave-uniform, so no lane leaves a loop
//            another lane still exchanges data in.  The wavefronts of a workgroup never meet: there is no workgroup barrier.
// The lane-to-pixel mapping is fixed by h alone (position p = lane + 64 k), nothing is accumulated across lanes but by the
// butterfly, nothing is atomic: a corner's outputs are a pure function of its image, start and (h, max_iterations, eps).
// Every pixel index is clamped to the image; the inside test makes the clamp a no-op, the clamp stays as the guard.
#include <cmath>
#include "ccal_call.hpp"
#include "ccal_image_device.hpp"

namespace ccal {

constexpr int kCornerWaves = 4;              // wavefronts (= corners in flight) per workgroup
constexpr int kCornerMaxHalf = 15;           // half_win 1 .. 15: a patch of at most 33 x 33 doubles per wavefront
constexpr int kCornerWTab = 2 * kCornerMaxHalf + 2;      // the weight table's room per wavefront (31 used)

// CornerArgs: ccal_internal.hpp

template <class T>
__global__ __launch_bounds__(64 * kCornerWaves) void k_corner_refine(const CornerArgs a) {
    extern __shared__ double corner_lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * kCornerWaves + wave;
    if (g >= a.n) return;
    const int h = a.h, side = 2 * h + 1, ps = 2 * h + 3;
    double* P = corner_lds + (size_t)wave * (size_t)(ps * ps + kCornerWTab);
    double* w1 = P + ps * ps;

    const T* img = static_cast<const T*>(a.img) + (int64_t)image_of_row(a.off, a.n_img, g) * a.W * a.H;
    const int32_t W = a.W, H = a.H;

    if (lane < side) { const double t = (double)(lane - h) / (double)h; w1[lane] = exp(-(t * t)); }
    wave_handoff();
    double sw = 0.0;
    for (int i = 0; i < side; ++i) sw += w1[i];
    const double sum_w = sw * sw;

    const double c0x = a.xy[2 * g], c0y = a.xy[2 * g + 1];
    double cx = c0x, cy = c0y;
    double lam = __builtin_nan("");
    int it = 0, status;
    const double lo_x = (double)(h + 1), hi_x = (double)(W - 2 - h), hi_y = (double)(H - 2 - h);
    for (;;) {
        // false for NaN; +-inf fail one of the two sides
        const bool inside = cx >= lo_x && cx <= hi_x && cy >= lo_x && cy <= hi_y;
        if (!inside) { status = CCAL_NO_RESULT; break; }
        for (int p = lane; p < ps * ps; p += 64) {
            const int pj = p / ps, pi = p - pj * ps;
            P[p] = image_sample(img, W, H, cx + (double)(pi - h - 1), cy + (double)(pj - h - 1));
        }
        wave_handoff();
        double sa = 0.0, sb = 0.0, sd = 0.0, su = 0.0, sv = 0.0;
        for (int p = lane; p < side * side; p += 64) {
            const int wj = p / side, wi = p - wj * side;
            const double* q = P + (wj + 1) * ps + (wi + 1);
            const double gx = q[1] - q[-1], gy = q[ps] - q[-ps];
            const double w = w1[wi] * w1[wj];
            const double di = (double)(wi - h), dj = (double)(wj - h);
            const double xx = gx * gx, xy = gx * gy, yy = gy * gy;
            sa += w * xx; sb += w * xy; sd += w * yy;
            su += w * (xx * di + xy * dj);
            sv += w * (xy * di + yy * dj);
        }
        wave_handoff();                 // the next iterate's patch is written after every lane has read this one
        for (int off = 32; off > 0; off >>= 1) {
            sa += __shfl_xor(sa, off, 64); sb += __shfl_xor(sb, off, 64); sd += __shfl_xor(sd, off, 64);
            su += __shfl_xor(su, off, 64); sv += __shfl_xor(sv, off, 64);
        }
        const double tr = sa + sd, det = sa * sd - sb * sb;
        lam = (tr - sqrt((sa - sd) * (sa - sd) + 4.0 * sb * sb)) / (2.0 * sum_w);
        if (!(det > 1e-12 * (tr * tr))) { status = CCAL_ERR_NOT_PD; break; }
        const double dx = (sd * su - sb * sv) / det, dy = (sa * sv - sb * su) / det;
        cx += dx; cy += dy;
        ++it;
        const double e = sqrt(dx * dx + dy * dy);
        if (e <= a.eps) { status = CCAL_OK; break; }
        if (it >= a.max_it) { status = CCAL_ERR_NO_CONVERGENCE; break; }
    }
    if ((status == CCAL_OK || status == CCAL_ERR_NO_CONVERGENCE) && (fabs(cx - c0x) > (double)h || fabs(cy - c0y) > (double)h))
        status = CCAL_NO_RESULT;           // the window slid off the corner it was given
    if (status == CCAL_NO_RESULT || status == CCAL_ERR_NOT_PD) { cx = c0x; cy = c0y; }
    if (lane == 0) {
        a.xy[2 * g] = cx; a.xy[2 * g + 1] = cy;
        a.status[g] = status; a.iters[g] = it; a.lam[g] = lam;
    }
}

const char* corners_bad_params(int half_win, int max_iterations, double eps) {
    if (half_win < 1 || half_win > kCornerMaxHalf) return "half_win outside 1 .. 15";
    if (max_iterations < 1) return "max_iterations < 1";
    if (!(eps >= 0.0) || !std::isfinite(eps)) return "eps negative or not finite";
    return nullptr;
}

hipError_t corners_enqueue(hipStream_t s, int dtype, const CornerArgs& a) {
    const int ps = 2 * a.h + 3;
    const size_t lds = sizeof(double) * (size_t)kCornerWaves * (size_t)(ps * ps + kCornerWTab);
    const dim3 grid((unsigned)(((size_t)a.n + kCornerWaves - 1) / kCornerWaves));
    for_pix_type(dtype, [&](auto t) { hipLaunchKernelGGL(k_corner_refine<decltype(t)>, grid, dim3(64 * kCornerWaves), lds, s, a); });
    return hipGetLastError();
}

namespace {

int corners_call(ccal_ctx* ctx, const char* where, const GreyBatch& b, const int64_t* offsets, double* xy_io, int half_win, int max_iterations,
                 double eps, int32_t* status_out, int32_t* iters_out, double* lambda_min_out) {
    const BadArg bad{ ctx, where };
    if (const char* what = corners_bad_params(half_win, max_iterations, eps)) return bad(what);
    if (const char* what = b.bad()) return bad(what);
    const int n_img = b.n_img;
    if (n_img == 0) return CCAL_OK;
    if (!b.images || !offsets || !status_out) return bad("NULL argument");
    if (check_offsets(ctx, where, "offsets", offsets, (size_t)n_img, 0)) return CCAL_ERR_INVALID_ARG;
    const int64_t n64 = offsets[n_img];
    if (n64 > (int64_t)INT32_MAX) return bad("more than 2^31 - 1 corners");
    if (n64 == 0) return CCAL_OK;
    if (!xy_io) return bad("NULL argument");
    const size_t n = (size_t)n64, ni = (size_t)n_img;

    // one block: offsets | images (host call) | corners, lambda_min | status, iterations
    CallBlock blk(ctx);
    const auto s_off = blk.add<int64_t>(ni + 1);
    const auto s_img = blk.add<char>(b.staged_bytes(ni));
    const auto s_xy = blk.add<double>(2 * n);
    const auto s_lam = blk.add<double>(n);
    const auto s_status = blk.add<int32_t>(n);
    const auto s_iters = blk.add<int32_t>(n);
    if (!blk.alloc()) return blk.finish(where);
    blk.poison(s_xy, s_lam);
    CornerArgs a = {};
    a.off = blk.at(s_off); a.xy = blk.at(s_xy); a.lam = blk.at(s_lam); a.status = blk.at(s_status); a.iters = blk.at(s_iters);
    a.n = n64; a.W = b.width; a.H = b.height; a.n_img = n_img; a.h = half_win; a.max_it = max_iterations; a.eps = eps;
    blk.upload(s_off, offsets, ni + 1);
    a.img = b.chunk(blk, s_img, 0, ni);
    blk.upload(s_xy, xy_io, 2 * n);
    if (blk.ok()) blk.note(corners_enqueue(ctx->stream, b.dtype, a));
    blk.download(xy_io, a.xy, 2 * n);
    blk.download(status_out, a.status, n);
    blk.download(iters_out, a.iters, n);
    blk.download(lambda_min_out, a.lam, n);
    return blk.finish(where);
}

}  // namespace
}  // namespace ccal

using namespace ccal;

extern "C" {

int ccal_refine_corners_batch(ccal_ctx* ctx, int dtype, int width, int height, int n_img, const void* images, const int64_t* offsets,
                              double* xy_io, int half_win, int max_iterations, double eps, int32_t* status_out, int32_t* iters_out,
                              double* lambda_min_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    return corners_call(ctx, "ccal_refine_corners_batch", GreyBatch{ dtype, width, height, n_img, images, false }, offsets, xy_io,
                        half_win, max_iterations, eps, status_out, iters_out, lambda_min_out);
    CCAL_API_CATCH(ctx)
}

int ccal_refine_corners_dev(ccal_ctx* ctx, int dtype, int width, int height, int n_img, const void* images_dev, const int64_t* offsets,
                            double* xy_io, int half_win, int max_iterations, double eps, int32_t* status_out, int32_t* iters_out,
                            double* lambda_min_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    return corners_call(ctx, "ccal_refine_corners_dev", GreyBatch{ dtype, width, height, n_img, images_dev, true }, offsets, xy_io,
                        half_win, max_iterations, eps, status_out, iters_out, lambda_min_out);
    CCAL_API_CATCH(ctx)
}

}  // extern "C"

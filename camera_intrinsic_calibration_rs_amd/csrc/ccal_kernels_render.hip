// Rendering calibration targets through the camera models (ccal_render_targets_batch / _dev): every pixel of a batch of grey images
// the mean of s x s rays, each unprojected through the model, intersected with the target's plane and classified black, white or
// background, by the rule stated at the entry points in include/ccal.h.  All images of a chunk in ONE launch:
//   k_render<MODEL, TARGET, T>  a lane owns 4 (u8) or 2 (u16) horizontally adjacent pixels of one row and stores them as one dword;
//            the 64 lanes of a wavefront cover a compact tile of 8 lanes x 8 rows (32 x 8 or 16 x 8 pixels), the four wavefronts of a
//            workgroup 2 x 2 such tiles: the lanes of a wavefront look at the same few squares or tags.  blockIdx.x walks the tiles
//            of an image, blockIdx.y the images.
//   staging  the codes of the tags on the board (first_id .. first_id + tag_rows tag_cols - 1) and the s sub-pixel offsets go into LDS
//            once per workgroup; an image's R and R^T t are read wave-uniformly, once per image.
//   stores   a lane whose pixels end at the image's right edge, or whose first pixel is not on a dword boundary (rows of a width that is
//            no multiple of 4 bytes), stores its own pixels one by one: no lane ever writes a byte it does not own.
//            This store is the renderer's own; the pixel table, the quantisation and the tile arithmetic are ccal_pix.hpp's.
// No atomics, no cross-lane traffic: a pixel is a pure function of the model, the target, the options and its image's pose.
// This unit is compiled with -ffp-contract=off (csrc/Makefile): the plane intersection and the lattice arithmetic round every
// product and sum on their own, as tests/render_ref.py, the numpy f64 yardstick, does.
#include <cmath>
#include <cstring>
#include <vector>
#include "ccal_call.hpp"
#include "ccal_device.hpp"
#include "ccal_model_inverse.hpp"
#include "ccal_photo.hpp"
#include "ccal_pix.hpp"

namespace ccal {

constexpr int kRenderMaxSS = 8;                       // supersample 1 .. 8
constexpr int kRenderMaxTags = 4096;                  // tags on a board: their codes are staged in LDS (32 KB)
constexpr size_t kRenderChunkBytes = (size_t)256 << 20;   // the block one launch of the host form should need
constexpr int kRenderTileRows = 16, kRenderTileLanes = 16;  // a workgroup: 16 rows of 16 lanes (2 x 2 wavefronts of 8 x 8)

struct RenderArgs {
    double th[CCAL_PMAX];
    ModelRt rt;
    const double* pose;                // [n_img][12]: R row-major, then R^T t
    const unsigned long long* codes;   // [n_tags]: the codes of the board's tags, tag (r, c) at r tag_cols + c
    void* out;                         // [n_img][H][W]
    int32_t W, H, n_img, s;
    int32_t tiles_x, n_tags;
    double black, white, background;
    // the sheet: x_lo <= X <= x_hi and y_lo <= Y <= y_hi (Y counted downwards for the AprilGrid)
    double x_lo, x_hi, y_lo, y_hi;
    // checkerboard
    double square; int32_t cols, rows;
    // AprilGrid
    double size, pitch; int32_t tag_cols, tag_rows, d, border;
};

enum { kClassB = 0, kClassW = 1, kClassG = 2 };

// the class of the plane point (X, Y): include/ccal.h, "The two patterns"
template <int TARGET>
__device__ __forceinline__ int target_class(const RenderArgs& a, const unsigned long long* codes, double X, double Y) {
    if constexpr (TARGET == CCAL_TARGET_CHECKERBOARD) {
        if (!(X >= a.x_lo && X <= a.x_hi && Y >= a.y_lo && Y <= a.y_hi)) return kClassG;
        const double i = floor(X / a.square) + 1.0, j = floor(Y / a.square) + 1.0;
        const bool on = i >= 0.0 && i <= (double)a.cols && j >= 0.0 && j <= (double)a.rows;
        const double half = (i + j) * 0.5;                // i + j is an integer: even exactly when its half is one
        return (on && floor(half) == half) ? kClassB : kClassW;
    } else {
        const double Yd = -Y;                             // counted downwards from the first row's top edge
        if (!(X >= a.x_lo && X <= a.x_hi && Yd >= a.y_lo && Yd <= a.y_hi)) return kClassG;
        const double c = floor(X / a.pitch), r = floor(Yd / a.pitch);
        const double u = (X - c * a.pitch) / a.size, v = (Yd - r * a.pitch) / a.size;
        const bool in_c = c >= 0.0 && c < (double)a.tag_cols, in_r = r >= 0.0 && r < (double)a.tag_rows;
        if (in_c && in_r && u < 1.0 && v < 1.0) {
            const int n = a.d + 2 * a.border;
            const int cu = min(max((int)floor(u * (double)n), 0), n - 1) - a.border;
            const int cv = min(max((int)floor(v * (double)n), 0), n - 1) - a.border;
            if (cu < 0 || cu >= a.d || cv < 0 || cv >= a.d) return kClassB;            // the border ring
            const unsigned long long code = codes[(int)r * a.tag_cols + (int)c];
            return (int)((code >> (a.d * a.d - 1 - (cv * a.d + cu))) & 1ull);           // bit 1: white
        }
        const bool gap = u >= 1.0 && v >= 1.0 && c >= -1.0 && c < (double)a.tag_cols && r >= -1.0 && r < (double)a.tag_rows;
        return gap ? kClassB : kClassW;
    }
}

template <int MODEL, int TARGET, class T>
__global__ __launch_bounds__(256) void k_render(const RenderArgs a) {
    constexpr int PX = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
    extern __shared__ unsigned long long lds_codes[];     // [n_tags], then the s sub-pixel offsets
    double* sub = reinterpret_cast<double*>(lds_codes + a.n_tags);
    for (int i = threadIdx.x; i < a.n_tags; i += 256) lds_codes[i] = a.codes[i];
    if ((int)threadIdx.x < a.s) sub[threadIdx.x] = ((double)threadIdx.x + 0.5) / (double)a.s - 0.5;
    __syncthreads();

    const TileAt t = tile_at(a.tiles_x, kRenderTileLanes * PX, kRenderTileRows);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lx = (wave & 1) * 8 + (lane & 7), ly = (wave >> 1) * 8 + (lane >> 3);
    const int x0 = t.x_t + lx * PX, y = t.y_t + ly;
    if (x0 >= a.W || y >= a.H) return;                    // after the only barrier

    double th[th_len<MODEL>()];
#pragma unroll
    for (int i = 0; i < model_np(MODEL); ++i) th[i] = a.th[i];
    th[model_np(MODEL)] = a.rt.kb4_eps;
    const double ss = (double)(a.s * a.s);
    const int n_ray = a.s * a.s;

    for (int img = blockIdx.y; img < a.n_img; img += gridDim.y) {
        const double* P = a.pose + 12 * (size_t)img;      // wave-uniform
        const double r00 = P[0], r01 = P[1], r02 = P[2], r10 = P[3], r11 = P[4], r12 = P[5], r20 = P[6], r21 = P[7], r22 = P[8];
        const double tbx = P[9], tby = P[10], tbz = P[11];
        uint32_t word = 0;
        for (int k = 0; k < PX; ++k) {
            int n_b = 0, n_w = 0;
            const double px = (double)(x0 + k), py = (double)y;
            for (int b = 0; b < a.s; ++b) {
                const double v = py + sub[b];
                for (int c = 0; c < a.s; ++c) {
                    const double u = px + sub[c];
                    double rx, ry, rz;
                    int cls = kClassG;
                    if (unproject_ray<MODEL>(th, a.rt.unproject_eps, u, v, rx, ry, rz)) {
                        const double dx = r00 * rx + r10 * ry + r20 * rz;
                        const double dy = r01 * rx + r11 * ry + r21 * rz;
                        const double dz = r02 * rx + r12 * ry + r22 * rz;
                        const double kk = tbz / dz;
                        if (kk > 0.0 && kk <= 1.79769313486231570815e308)          // finite and positive; false for NaN
                            cls = target_class<TARGET>(a, lds_codes, kk * dx - tbx, kk * dy - tby);
                    }
                    n_b += cls == kClassB; n_w += cls == kClassW;
                }
            }
            const double lum = (((double)n_b * a.black + (double)n_w * a.white) + (double)(n_ray - n_b - n_w) * a.background) / ss;
            word |= pix_quantise<T>(lum) << (BITS * k);
        }
        T* dst = static_cast<T*>(a.out) + ((int64_t)img * a.H + y) * a.W + x0;
        if (x0 + PX <= a.W && (reinterpret_cast<uintptr_t>(dst) & 3u) == 0) *reinterpret_cast<uint32_t*>(dst) = word;
        else
            for (int k = 0; k < PX && x0 + k < a.W; ++k) dst[k] = (T)(word >> (BITS * k));
    }
}

namespace {

template <int MODEL>
void render_launch_m(int kind, int dtype, dim3 grid, size_t lds, hipStream_t st, const RenderArgs& a) {
    for_pix_type(dtype, [&](auto t) {
        if (kind == CCAL_TARGET_APRILGRID) hipLaunchKernelGGL((k_render<MODEL, CCAL_TARGET_APRILGRID, decltype(t)>), grid, dim3(256), lds, st, a);
        else hipLaunchKernelGGL((k_render<MODEL, CCAL_TARGET_CHECKERBOARD, decltype(t)>), grid, dim3(256), lds, st, a);
    });
}
hipError_t render_enqueue(int model, int kind, int dtype, hipStream_t st, RenderArgs a) {
    const TileGrid tg = tile_grid(a.W, a.H, kRenderTileLanes * (dtype == CCAL_PIX_U16 ? 2 : 4), kRenderTileRows, a.n_img);
    a.tiles_x = tg.tiles_x;
    const size_t lds = sizeof(unsigned long long) * (size_t)a.n_tags + sizeof(double) * kRenderMaxSS;
    switch (model) {
        case kUCM: render_launch_m<kUCM>(kind, dtype, tg.grid, lds, st, a); break;
        case kEUCM: render_launch_m<kEUCM>(kind, dtype, tg.grid, lds, st, a); break;
        case kKB4: render_launch_m<kKB4>(kind, dtype, tg.grid, lds, st, a); break;
        default: render_launch_m<kOCV5>(kind, dtype, tg.grid, lds, st, a); break;
    }
    return hipGetLastError();
}

// rvec, tvec (board -> camera) -> R row-major and R^T t, in f64: the Rodrigues formula R = I + sin(a) K + (1 - cos(a)) K K with
// K = [rvec / a]x, the identity for a < 1e-12
void pose_to_rt(const double* p, double* out) {
    const double a = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
    double R[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };
    if (!(a < 1e-12)) {
        const double kx = p[0] / a, ky = p[1] / a, kz = p[2] / a, s = std::sin(a), c1 = 1.0 - std::cos(a);
        const double K[9] = { 0.0, -kz, ky, kz, 0.0, -kx, -ky, kx, 0.0 };
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const double kk = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
                R[3 * i + j] = (i == j ? 1.0 : 0.0) + s * K[3 * i + j] + c1 * kk;
            }
    }
    std::memcpy(out, R, sizeof(R));
    for (int j = 0; j < 3; ++j) out[9 + j] = R[j] * p[3] + R[3 + j] * p[4] + R[6 + j] * p[5];
}

// with_photo: the ideal images are rendered at CCAL_PIX_U16 chunk by chunk into a slice of the block and go through the photometric
// stage (ccal_kernels_photo.hip) into the destination; without it the render writes the destination itself, as it always did
int render_call(ccal_ctx* ctx, const char* where, bool on_device, int model, const double* params, int dtype, int width, int height, int n_img,
                const double* poses, const ccal_render_target* tg, const ccal_render_opts* o, void* out, bool with_photo = false,
                const ccal_photo_opts* photo = nullptr) {
    const BadArg bad{ ctx, where };
    if (!params) return bad("params is NULL");
    if (!tg) return bad("target is NULL");
    if (!o) return bad("opts is NULL");
    const int rc = check_model(ctx, model, where);
    if (rc != CCAL_OK) return rc;
    if (const char* what = GreyBatch{ dtype, width, height, n_img, nullptr, on_device }.bad()) return bad(what);
    RenderArgs a = {};
    int n_tags = 0;
    if (tg->kind == CCAL_TARGET_CHECKERBOARD) {
        if (!(tg->square > 0.0) || !std::isfinite(tg->square)) return bad("square is not finite and positive");
        if (tg->cols < 1 || tg->rows < 1) return bad("cols or rows < 1");
        a.square = tg->square; a.cols = tg->cols; a.rows = tg->rows;
        a.x_lo = -tg->square - o->margin; a.x_hi = (double)tg->cols * tg->square + o->margin;
        a.y_lo = -tg->square - o->margin; a.y_hi = (double)tg->rows * tg->square + o->margin;
    } else if (tg->kind == CCAL_TARGET_APRILGRID) {
        if (!(tg->tag_size > 0.0) || !std::isfinite(tg->tag_size)) return bad("tag_size is not finite and positive");
        if (!(tg->tag_spacing > 0.0) || !std::isfinite(tg->tag_spacing)) return bad("tag_spacing is not finite and positive");
        if (tg->tag_rows < 1 || tg->tag_cols < 1) return bad("tag_rows or tag_cols < 1");
        if ((int64_t)tg->tag_rows * tg->tag_cols > kRenderMaxTags) return bad("more than 4096 tags (tag_rows * tag_cols)");
        int d = 0;
        while (d * d < tg->family_bits) ++d;
        if (tg->family_bits < 1 || tg->family_bits > 64 || d * d != tg->family_bits) return bad("family_bits is not a square in 1 .. 64");
        if (tg->border < 1) return bad("border < 1");
        if (tg->first_id < 0) return bad("first_id < 0");
        n_tags = tg->tag_rows * tg->tag_cols;
        if ((int64_t)tg->n_codes < (int64_t)tg->first_id + n_tags) return bad("n_codes: fewer codes than first_id + tag_rows * tag_cols");
        a.size = tg->tag_size; a.pitch = tg->tag_size * (1.0 + tg->tag_spacing);
        a.tag_cols = tg->tag_cols; a.tag_rows = tg->tag_rows; a.d = d; a.border = tg->border;
        const double gap = tg->tag_spacing * tg->tag_size;
        a.x_lo = -gap - o->margin; a.x_hi = (double)tg->tag_cols * a.pitch + o->margin;
        a.y_lo = -gap - o->margin; a.y_hi = (double)tg->tag_rows * a.pitch + o->margin;
    } else return bad("target kind is neither CCAL_TARGET_CHECKERBOARD nor CCAL_TARGET_APRILGRID");
    // the options after the target: a default margin is made from the target's sizes
    if (o->supersample < 1 || o->supersample > kRenderMaxSS) return bad("supersample outside 1 .. 8");
    if (!std::isfinite(o->black) || !std::isfinite(o->white) || !std::isfinite(o->background)) return bad("black, white or background is not finite");
    if (!(o->margin >= 0.0)) return bad("margin is negative or not a number");
    PhotoTables tables;
    if (with_photo) {
        if (!photo) return bad("photo is NULL");
        if (const char* what = photo_check(photo, &tables)) return bad(what);
    }
    if (n_img == 0) return CCAL_OK;
    if (!poses) return bad("poses is NULL");
    if (!out) return bad("the output pointer is NULL");
    if (n_tags && !tg->codes) return bad("codes is NULL");

    canonical_theta(ctx, model, params, a.th, &a.rt);
    a.W = width; a.H = height; a.s = o->supersample; a.n_tags = n_tags;
    a.black = o->black; a.white = o->white; a.background = o->background;
    std::vector<double> rt(12 * (size_t)n_img);
    for (int k = 0; k < n_img; ++k) pose_to_rt(poses + 6 * (size_t)k, rt.data() + 12 * (size_t)k);

    // the host form goes chunk by chunk through one staged block of images; the device form writes where the caller says.  With the
    // photometric stage both forms go chunk by chunk through one block of u16 ideal images, whose bytes the limit then counts
    const size_t img_bytes = (dtype == CCAL_PIX_U16 ? 2 : 1) * (size_t)width * (size_t)height;
    const size_t ideal_bytes = 2 * (size_t)width * (size_t)height;
    const size_t limit = test_chunk_bytes("CCAL_TEST_RENDER_CHUNK_BYTES", kRenderChunkBytes);
    const size_t per = on_device && !with_photo ? (size_t)n_img
                                                : std::min<size_t>((size_t)n_img, std::max<size_t>(limit / (with_photo ? ideal_bytes : img_bytes), 1));
    CallBlock blk(ctx);
    const auto s_pose = blk.add<double>(12 * (size_t)n_img);
    const auto s_codes = blk.add<unsigned long long>((size_t)n_tags);
    const auto s_img = blk.add<char>(on_device ? 0 : img_bytes * per);
    const auto s_ideal = blk.add<char>(with_photo ? ideal_bytes * per : 0);
    if (!blk.alloc()) return blk.finish(where);
    blk.upload(s_pose, rt.data(), rt.size());
    if (n_tags) blk.upload(s_codes, tg->codes + tg->first_id, (size_t)n_tags);
    a.codes = blk.at(s_codes);
    for (size_t k0 = 0; k0 < (size_t)n_img && blk.ok(); k0 += per) {
        const size_t m = std::min(per, (size_t)n_img - k0);
        a.pose = blk.at(s_pose) + 12 * k0; a.n_img = (int32_t)m;
        void* const dst = on_device ? static_cast<void*>(static_cast<char*>(out) + k0 * img_bytes) : static_cast<void*>(blk.at(s_img));
        a.out = with_photo ? static_cast<void*>(blk.at(s_ideal)) : dst;
        blk.note(render_enqueue(model, tg->kind, with_photo ? (int)CCAL_PIX_U16 : dtype, ctx->stream, a));
        if (with_photo && blk.ok())                      // an image's noise index is its index in the call
            blk.note(photo_enqueue(ctx->stream, tables, *photo, CCAL_PIX_U16, dtype, width, height, (int)m,
                                   photo->seed + (uint64_t)photo->first_index + (uint64_t)k0, a.out, dst));
        if (!on_device) blk.download(static_cast<char*>(out) + k0 * img_bytes, blk.at(s_img), img_bytes * m);
    }                                                    // the next chunk's launch follows this copy on the same stream
    return blk.finish(where);
}

}  // namespace
}  // namespace ccal

using namespace ccal;

extern "C" {

int ccal_render_set_defaults(const ccal_render_target* target, ccal_render_opts* opts) {
    if (!target || !opts) return CCAL_ERR_INVALID_ARG;
    opts->supersample = 4; opts->reserved_ = 0;
    opts->black = 40.0; opts->white = 215.0; opts->background = 0.0;
    opts->margin = target->kind == CCAL_TARGET_APRILGRID ? target->tag_size * (1.0 + target->tag_spacing) : target->square;
    return CCAL_OK;
}

int ccal_render_targets_batch(ccal_ctx* ctx, int model, const double* params, int dtype, int width, int height, int n_img,
                              const double* poses, const ccal_render_target* target, const ccal_render_opts* opts, void* images_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    return render_call(ctx, "ccal_render_targets_batch", false, model, params, dtype, width, height, n_img, poses, target, opts, images_out);
    CCAL_API_CATCH(ctx)
}

int ccal_render_targets_dev(ccal_ctx* ctx, int model, const double* params, int dtype, int width, int height, int n_img,
                            const double* poses, const ccal_render_target* target, const ccal_render_opts* opts, void* images_out_dev) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    return render_call(ctx, "ccal_render_targets_dev", true, model, params, dtype, width, height, n_img, poses, target, opts, images_out_dev);
    CCAL_API_CATCH(ctx)
}

int ccal_render_photo_targets(ccal_ctx* ctx, int model, const double* params, int dtype, int width, int height, int n_img, const double* poses,
                              const ccal_render_target* target, const ccal_render_opts* opts, const ccal_photo_opts* photo, void* images_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    return render_call(ctx, "ccal_render_photo_targets", false, model, params, dtype, width, height, n_img, poses, target, opts, images_out, true, photo);
    CCAL_API_CATCH(ctx)
}

int ccal_render_photo_targets_dev(ccal_ctx* ctx, int model, const double* params, int dtype, int width, int height, int n_img, const double* poses,
                                  const ccal_render_target* target, const ccal_render_opts* opts, const ccal_photo_opts* photo,
                                  void* images_out_dev) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    return render_call(ctx, "ccal_render_photo_targets_dev", true, model, params, dtype, width, height, n_img, poses, target, opts, images_out_dev, true,
                       photo);
    CCAL_API_CATCH(ctx)
}

}  // extern "C"

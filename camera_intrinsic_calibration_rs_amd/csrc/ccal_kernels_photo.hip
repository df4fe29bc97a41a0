// The photometric stage (ccal_photo_apply_dev; ccal_render_photo_targets / _dev through the renderer's host code): from ideal
// irradiance to pixels - Gaussian lens blur, vignetting, exposure, read and shot noise, quantisation - by the rule stated at the
// entry points in include/ccal.h.  All images of a call in ONE launch:
//   k_photo<S, D>  a workgroup owns an output tile of 64 x 16 pixels of one image; blockIdx.x walks the tiles of an image,
//            blockIdx.y the images.  The radius, the taps and the noise table arrive by value in the kernel's arguments and go into
//            LDS once per workgroup: no device allocation, nothing staged.
//   tile     the source tile with a halo of r pixels on every side, clamped to the image, goes into LDS as u16 (a u8 source times 257).
//   rows     the horizontal pass: lane = x, a wavefront per tile row (halo rows included), f64 rows in LDS.
//   columns  the vertical pass: lane = x again, so that the 64 lanes of a wavefront read 64 consecutive doubles of one f64 row - no
//            bank conflict; a lane owns four rows of its column and reads every f64 row it needs once.  r = 0 skips both passes and
//            reads the pixel from the source.
//   pixel    steps c to g in the lane that holds B(x, y).  The noise is counter-based: three splitmix64 finalisers per pixel, keyed by
//            the image's stream and the pixel's index - no state, no atomics, no order.
//   stores   store_pixel_group: dwords of 4 u8 or 2 u16, pixel by pixel at the right edge and on unaligned rows; no lane writes
//            outside the image.  It, the pixel table, the tile's load, the quantisation and the tile arithmetic are ccal_pix.hpp's,
//            shared with k_normalize.
// This unit is compiled with -ffp-contract=off (csrc/Makefile): every product and sum rounds on its own, as tests/photo_ref.py, the
// numpy yardstick, does; the device is held to it bit for bit.
#include <algorithm>
#include <cmath>
#include "ccal_call.hpp"
#include "ccal_photo.hpp"
#include "ccal_pix.hpp"

namespace ccal {

constexpr int kPhotoTileW = 64, kPhotoTileH = 16, kPhotoRows = 4;   // a workgroup: 4 wavefronts, each 64 columns x 4 rows
constexpr int kPhotoMaxR = CCAL_PHOTO_MAX_RADIUS;
static_assert(kPhotoTileH == 4 * kPhotoRows, "four wavefronts cover the tile's rows");

struct PhotoArgs {
    PhotoTables t;                     // 273 doubles: under the 4 KB of a kernel's arguments
    const void* src;                   // [n_img][H][W]
    void* dst;                         // [n_img][H][W]
    int32_t W, H, n_img, tiles_x;
    double vignette, gain, cx, cy, den;   // den = cx cx + cy cy, 0 for a 1 x 1 image
    unsigned long long stream0;        // seed + first_index + the index in the call of the launch's first image
    int32_t noisy, reserved_;          // 0: the noise table is all zeros, Y = V
};
static_assert(sizeof(PhotoArgs) <= 4096, "the kernel's arguments");

__host__ __device__ __forceinline__ unsigned long long photo_mix(unsigned long long a) {
    a ^= a >> 30; a *= 0xBF58476D1CE4E5B9ull;
    a ^= a >> 27; a *= 0x94D049BB133111EBull;
    a ^= a >> 31;
    return a;
}
__device__ __forceinline__ unsigned photo_fields(unsigned long long w) {
    return (unsigned)(w & 0xFFFFull) + (unsigned)((w >> 16) & 0xFFFFull) + (unsigned)((w >> 32) & 0xFFFFull) + (unsigned)(w >> 48);
}

// LDS: the noise table [256], the taps [24 with padding], the f64 rows [TH + 2 r][TW], the u16 tile [TH + 2 r][TW + 2 r]
__host__ __device__ inline size_t photo_lds_bytes(int r) {
    const size_t ih = (size_t)(kPhotoTileH + 2 * r), iw = (size_t)(kPhotoTileW + 2 * r);
    return r == 0 ? sizeof(double) * (256 + 24) : sizeof(double) * (256 + 24 + ih * kPhotoTileW) + ((sizeof(uint16_t) * ih * iw + 15) & ~(size_t)15);
}

template <class S, class D>
__global__ __launch_bounds__(256) void k_photo(const PhotoArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds_photo[];
    double* sig_s = lds_photo;                                       // [256]
    double* tap_s = lds_photo + 256;                                 // [17], 24 reserved
    double* rows_s = lds_photo + 256 + 24;                           // [ih][TW]
    const int r = a.t.radius;
    const int ih = kPhotoTileH + 2 * r, iw = kPhotoTileW + 2 * r;
    uint16_t* tile_s = reinterpret_cast<uint16_t*>(rows_s + (size_t)ih * kPhotoTileW);   // [ih][iw]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    sig_s[tid] = a.t.sigma[tid];
    if (tid <= kPhotoMaxR) tap_s[tid] = a.t.taps[tid];

    const TileAt t = tile_at(a.tiles_x, kPhotoTileW, kPhotoTileH);         // the tile's first pixel: (t.x_t, t.y_t)
    const int x = t.x_t + lane, y0 = t.y_t + wave * kPhotoRows;            // this lane's column and its first row
    const int xc = min(x, a.W - 1);                                        // a lane beyond the right edge works on the edge and stores nothing
    const S* src = static_cast<const S*>(a.src);
    D* dst = static_cast<D*>(a.dst);
    const int64_t n_pix = (int64_t)a.W * a.H;

    for (int img = blockIdx.y; img < a.n_img; img += gridDim.y) {
        const S* I = src + (int64_t)img * n_pix;
        double B[kPhotoRows];
        if (r == 0) {
            __syncthreads();                                               // the tables, on the first image
#pragma unroll
            for (int i = 0; i < kPhotoRows; ++i) B[i] = (double)((unsigned)I[(int64_t)min(y0 + i, a.H - 1) * a.W + xc] * Pix<S>::up);
        } else {
            load_halo_tile<S>(tile_s, I, a.W, a.H, t.x_t, t.y_t, r, iw, ih, tid);
            __syncthreads();
            // a: rows.  tile column lane + r + j is pixel x + j
            for (int ty = wave; ty < ih; ty += 4) {
                const uint16_t* row = tile_s + ty * iw + lane;
                double acc = 0.0;
                for (int j = -r; j <= r; ++j) acc = acc + tap_s[abs(j)] * (double)row[r + j];
                rows_s[ty * kPhotoTileW + lane] = acc;
            }
            __syncthreads();
            // b: columns.  f64 row ty is image row y_t - r + ty: output row y0 + i takes the rows wave * 4 + i + (0 .. 2 r), tap |m - r|
#pragma unroll
            for (int i = 0; i < kPhotoRows; ++i) B[i] = 0.0;
            const double* col = rows_s + (wave * kPhotoRows) * kPhotoTileW + lane;
            for (int m = 0; m < kPhotoRows + 2 * r; ++m) {
                const double h = col[m * kPhotoTileW];
#pragma unroll
                for (int i = 0; i < kPhotoRows; ++i) {
                    const int j = m - i - r;                               // ascending in m for every i
                    if (j >= -r && j <= r) B[i] = B[i] + tap_s[abs(j)] * h;
                }
            }
        }
        const unsigned long long key = photo_mix(a.stream0 + (unsigned long long)img);
#pragma unroll
        for (int i = 0; i < kPhotoRows; ++i) {
            const int y = y0 + i;                                          // wave-uniform
            if (y >= a.H) break;
            // c
            const double dx = (double)x - a.cx, dy = (double)y - a.cy;
            const double rho2 = a.den > 0.0 ? (dx * dx + dy * dy) / a.den : 0.0;
            const double f = 1.0 + a.vignette * rho2;
            const double g = 1.0 / (f * f);
            const double V = ((B[i] / 257.0) * a.gain) * g;
            double Y = V;
            if (a.noisy) {
                // d
                const double Vc = fmin(fmax(V, 0.0), 255.0);
                const double fi = fmin(floor(Vc), 254.0);
                const int k = (int)fi;
                const double sig = sig_s[k] + (sig_s[k + 1] - sig_s[k]) * (Vc - fi);
                // e
                const unsigned long long at = key + 4ull * (unsigned long long)((int64_t)y * a.W + x);
                const unsigned S12 = photo_fields(photo_mix(at)) + photo_fields(photo_mix(at + 1ull)) + photo_fields(photo_mix(at + 2ull));
                const double z = (double)((int)S12 - 393210) / 65536.0;
                // f
                Y = V + sig * z;
            }
            // g
            const unsigned q = pix_quantise<D>(Y);
            // the group's pixels to its first lane; every lane of the wavefront is here
            store_pixel_group<D>(dst + ((int64_t)img * a.H + y) * a.W, x, lane, a.W, q);
        }
    }
}

namespace {

bool finite_nonneg(double v) { return v >= 0.0 && std::isfinite(v); }

}  // namespace

const char* photo_check(const ccal_photo_opts* o, PhotoTables* t) {
    if (!(o->blur_sigma >= 0.0 && o->blur_sigma <= 16.0 / 3.0)) return "blur_sigma is outside 0 .. 16/3";
    if (!finite_nonneg(o->vignette)) return "vignette is negative or not finite";
    if (!finite_nonneg(o->gain)) return "gain is negative or not finite";
    if (!finite_nonneg(o->noise_read)) return "noise_read is negative or not finite";
    if (!finite_nonneg(o->noise_shot)) return "noise_shot is negative or not finite";
    if (o->first_index < 0) return "first_index < 0";
    const double s = o->blur_sigma;
    const int r = (int)std::min(16.0, std::ceil(3.0 * s));
    t->radius = r; t->reserved_ = 0;
    for (int k = 0; k <= kPhotoMaxR; ++k) t->taps[k] = 0.0;
    if (r == 0) t->taps[0] = 1.0;
    else {
        double w[kPhotoMaxR + 1] = { 1.0 }, tail = 0.0;    // w_0 = 1 as written: -0 / (2 s s) is not a number once 2 s s underflows
        for (int k = 1; k <= r; ++k) w[k] = std::exp(-(double)(k * k) / (2.0 * s * s));
        for (int k = 1; k <= r; ++k) tail = tail + w[k];
        const double norm = w[0] + 2.0 * tail;
        for (int k = 0; k <= r; ++k) t->taps[k] = w[k] / norm;
    }
    for (int g = 0; g < 256; ++g) t->sigma[g] = std::sqrt(o->noise_read * o->noise_read + o->noise_shot * (double)g);
    return nullptr;
}

hipError_t photo_enqueue(hipStream_t st, const PhotoTables& tables, const ccal_photo_opts& o, int src_dtype, int dst_dtype, int width, int height,
                         int n_img, uint64_t stream0, const void* src, void* dst) {
    if (n_img <= 0) return hipSuccess;
    PhotoArgs a = {};
    a.t = tables; a.src = src; a.dst = dst;
    a.W = width; a.H = height; a.n_img = n_img;
    const TileGrid tg = tile_grid(width, height, kPhotoTileW, kPhotoTileH, n_img);
    a.tiles_x = tg.tiles_x;
    a.vignette = o.vignette; a.gain = o.gain;
    a.cx = (double)(width - 1) / 2.0; a.cy = (double)(height - 1) / 2.0;
    a.den = a.cx * a.cx + a.cy * a.cy;
    a.stream0 = stream0;
    a.noisy = (o.noise_read > 0.0 || o.noise_shot > 0.0) ? 1 : 0;
    const size_t lds = photo_lds_bytes(tables.radius);
    for_pix_type(src_dtype, [&](auto s) { for_pix_type(dst_dtype, [&](auto d) {
        hipLaunchKernelGGL((k_photo<decltype(s), decltype(d)>), tg.grid, dim3(256), lds, st, a);
    }); });
    return hipGetLastError();
}

}  // namespace ccal

using namespace ccal;

extern "C" {

int ccal_photo_set_defaults(ccal_photo_opts* photo) {
    if (!photo) return CCAL_ERR_INVALID_ARG;
    photo->blur_sigma = 0.0; photo->vignette = 0.0; photo->gain = 1.0;
    photo->noise_read = 0.0; photo->noise_shot = 0.0;
    photo->seed = 0; photo->first_index = 0;
    return CCAL_OK;
}

int ccal_photo_tables(const ccal_photo_opts* photo, int32_t* radius_out, double* taps_out, double* sigma_out) {
    if (!photo || !radius_out || !taps_out || !sigma_out) return CCAL_ERR_INVALID_ARG;
    PhotoTables t;
    if (photo_check(photo, &t)) return CCAL_ERR_INVALID_ARG;
    *radius_out = t.radius;
    for (int k = 0; k <= kPhotoMaxR; ++k) taps_out[k] = t.taps[k];
    for (int g = 0; g < 256; ++g) sigma_out[g] = t.sigma[g];
    return CCAL_OK;
}

int ccal_photo_apply_dev(ccal_ctx* ctx, int src_dtype, int dst_dtype, int width, int height, int n_img, const void* src_dev, void* dst_dev,
                         const ccal_photo_opts* photo) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    const BadArg bad{ ctx, "ccal_photo_apply_dev" };
    if (!photo) return bad("photo is NULL");
    PhotoTables t;
    if (const char* what = photo_check(photo, &t)) return bad(what);
    const PairCheck pair = image_pair_check(src_dtype, dst_dtype, width, height, n_img, src_dev, dst_dev);
    if (!pair.go) return pair.what ? bad(pair.what) : CCAL_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, photo_enqueue(ctx->stream, t, *photo, src_dtype, dst_dtype, width, height, n_img, photo->seed + (uint64_t)photo->first_index,
                               src_dev, dst_dev));
    return CCAL_OK;
    CCAL_API_CATCH(ctx)
}

}  // extern "C"

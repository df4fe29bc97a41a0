// Local contrast normalisation (ccal_normalize_dev): every pixel minus the mean of its (2 r + 1)^2 window over the window's standard
// deviation, by the rule stated at the entry point in include/ccal.h - the window sums, the variance term and its square root in exact
// integers, one f64 division and one multiply-add (unfused) at the end.  All images of a call in ONE launch:
//   k_normalize<S, D, TH>  a workgroup owns an output tile of 64 x TH pixels of one image (TH = 32, or 16 at r > 16:
//            normalize_tile_h); blockIdx.x walks the tiles of an image, blockIdx.y the images.  No device allocation, nothing staged.
//   tile     the source tile with a halo of r pixels on every side, clamped to the image, goes into LDS as u16 (a u8 source times 257).
//   columns  the vertical pass FIRST, because a lane can keep RUNNING sums down a column: lane = a column of the tile, halo columns
//            included (64 + 2 r <= 128: two rounds); a wavefront owns TH / 4 consecutive output rows, sums I and I I over the 2 r + 1 tile
//            rows of its first and then lets one row enter and one leave per output row.  The sums are integers, so the order is
//            free and the running sums are exact.  The halo's redundancy - (TH + 2 r) / TH rows - thus falls on the pass that costs
//            O(1) per entry, not on the one that costs 2 r + 1.  Both column sums go into ONE u64 in LDS, the sum of I (< 2^23) in
//            the upper 24 bits, the sum of I I (< 2^39) in the lower 40: eight bytes per entry instead of twelve.
//   rows     the horizontal pass over the TH output rows only: lane = x, 2 r + 1 consecutive u64 of one row of column sums (no bank
//            conflict).  A wavefront reads the rows it wrote.
//   pixel    v = N S2 - S1 S1, its integer square root seeded from the f64 square root and corrected in integers both ways, the
//            floor N F, d = N I - S1, q = d / s, Y = 128 + amp q, the quantisation.
//   stores   store_pixel_group: dwords of 4 u8 or 2 u16, pixel by pixel at the right edge and on unaligned rows; no lane writes outside
//            the image.  It, the pixel table, the tile's load, the quantisation and the tile arithmetic are ccal_pix.hpp's, k_photo's too.
// This unit is compiled with -ffp-contract=off (csrc/Makefile): Y = 128 + amp q rounds the product and the sum on their own, as
// tests/normalize_ref.py, the numpy yardstick, does; the device is held to it bit for bit.
#include <algorithm>
#include <cmath>
#include "ccal_call.hpp"
#include "ccal_pix.hpp"

namespace ccal {

constexpr int kNormTileW = 64;
constexpr int kNormMaxR = CCAL_NORMALIZE_MAX_RADIUS;
constexpr unsigned long long kNormLow40 = (1ull << 40) - 1ull;

// the tile's height, a multiple of 4 (a wavefront owns a quarter of the rows): 32 rows up to r = 16, 16 beyond, where the smaller tile
// lets four workgroups share a CU's LDS instead of two (EXPERIMENTS.md).  -DCCAL_NORM_TILE_H=n forces one height: the A/B builds.
__host__ __device__ constexpr int normalize_tile_h(int r) {
#ifdef CCAL_NORM_TILE_H
    return CCAL_NORM_TILE_H;
#else
    return r <= 16 ? 32 : 16;
#endif
}
// LDS: the packed column sums [th][64 + 2 r] u64, then the u16 tile [th + 2 r][64 + 2 r]
__host__ __device__ constexpr size_t normalize_lds_bytes(int r) {
    const size_t th = (size_t)normalize_tile_h(r), ih = th + 2 * (size_t)r, iw = (size_t)(kNormTileW + 2 * r);
    return sizeof(unsigned long long) * th * iw + ((sizeof(uint16_t) * ih * iw + 15) & ~(size_t)15);
}
static_assert(normalize_lds_bytes(kNormMaxR) <= 65536 && normalize_lds_bytes(16) <= 65536, "the default limit of dynamic LDS");

struct NormArgs {
    const void* src;                   // [n_img][H][W]
    void* dst;                         // [n_img][H][W]
    int32_t W, H, n_img, tiles_x;
    int32_t r, reserved_;              // the radius
    unsigned long long n_win;          // N = (2 r + 1)^2
    unsigned long long floor_s;        // N F, F = max(1, rint(257 min_sigma))
    double amp;
};

// the largest s with s s <= v, v < 2^63: the seed's rounding does not reach the result
__device__ __forceinline__ unsigned long long norm_isqrt(unsigned long long v) {
    unsigned long long s = (unsigned long long)sqrt((double)v);
    while (s * s > v) --s;
    while ((s + 1ull) * (s + 1ull) <= v) ++s;
    return s;
}

template <class S, class D, int TH>
__global__ __launch_bounds__(256) void k_normalize(const NormArgs a) {
    static_assert(TH % 4 == 0 && TH >= 4, "four wavefronts cover the tile's rows");
    extern __shared__ __attribute__((aligned(16))) unsigned long long lds_norm[];
    constexpr int th = TH, rpw = TH / 4;                                    // rows per wavefront
    const int r = a.r;
    const int ih = th + 2 * r, iw = kNormTileW + 2 * r;
    unsigned long long* cols_s = lds_norm;                                  // [th][iw]
    uint16_t* tile_s = reinterpret_cast<uint16_t*>(cols_s + (size_t)th * iw);   // [ih][iw]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

    const TileAt t = tile_at(a.tiles_x, kNormTileW, th);                    // the tile's first pixel: (t.x_t, t.y_t)
    const int x = t.x_t + lane;                                             // a lane beyond the right edge works on clamped pixels and stores nothing
    const int k0 = wave * rpw;                                              // this wavefront's first output row of the tile
    const S* src = static_cast<const S*>(a.src);
    D* dst = static_cast<D*>(a.dst);
    const int64_t n_pix = (int64_t)a.W * a.H;

    for (int img = blockIdx.y; img < a.n_img; img += gridDim.y) {
        const S* I = src + (int64_t)img * n_pix;
        load_halo_tile<S>(tile_s, I, a.W, a.H, t.x_t, t.y_t, r, iw, ih, tid);
        __syncthreads();
        // columns.  tile row ty is image row y_t - r + ty: output row y_t + k takes the tile rows k .. k + 2 r
        for (int cx = lane; cx < iw; cx += 64) {
            const uint16_t* col = tile_s + k0 * iw + cx;
            unsigned c1 = 0u;
            unsigned long long c2 = 0ull;
            for (int m = 0; m <= 2 * r; ++m) {
                const unsigned p = col[m * iw];
                c1 += p;
                c2 += (unsigned long long)(p * p);                          // p < 2^16: the product fits 32 bits
            }
            cols_s[k0 * iw + cx] = ((unsigned long long)c1 << 40) | c2;
            for (int i = 1; i < rpw; ++i) {
#ifdef CCAL_NORM_PLAIN_COLUMNS                                              // the A/B of EXPERIMENTS.md: every row's sums from scratch
                c1 = 0u; c2 = 0ull;
                for (int m = 0; m <= 2 * r; ++m) {
                    const unsigned p = col[(i + m) * iw];
                    c1 += p;
                    c2 += (unsigned long long)(p * p);
                }
#else
                const unsigned in = col[(i + 2 * r) * iw], out = col[(i - 1) * iw];
                c1 += in; c1 -= out;
                c2 += (unsigned long long)(in * in); c2 -= (unsigned long long)(out * out);
#endif
                cols_s[(k0 + i) * iw + cx] = ((unsigned long long)c1 << 40) | c2;
            }
        }
        __syncthreads();
        // rows.  column-sum column lane + j, j = 0 .. 2 r, is pixel x - r + j
        for (int i = 0; i < rpw; ++i) {
            const int y = t.y_t + k0 + i;                                   // wave-uniform
            if (y >= a.H) break;
            const unsigned long long* row = cols_s + (k0 + i) * iw + lane;
            unsigned S1 = 0u;
            unsigned long long S2 = 0ull;
            for (int j = 0; j <= 2 * r; ++j) {
                const unsigned long long p = row[j];
                S1 += (unsigned)(p >> 40); S2 += p & kNormLow40;
            }
            const unsigned long long c = tile_s[(k0 + i + r) * iw + lane + r];
            const unsigned long long v = a.n_win * S2 - (unsigned long long)S1 * (unsigned long long)S1;
            const unsigned long long s = max(norm_isqrt(v), a.floor_s);
            const long long d = (long long)(a.n_win * c) - (long long)S1;
            const double q = (double)d / (double)s;
            const double Y = 128.0 + a.amp * q;
            const unsigned px = pix_quantise<D>(Y);
            store_pixel_group<D>(dst + ((int64_t)img * a.H + y) * a.W, x, lane, a.W, px);
        }
        __syncthreads();                                                    // the next image's tile overwrites what the rows read
    }
}

namespace {

// nullptr, or the message of the first option out of range
const char* normalize_check(const ccal_normalize_opts* o) {
    if (o->radius < 1 || o->radius > kNormMaxR) return "radius is outside 1 .. 32";
    if (!(o->min_sigma >= 0.0 && o->min_sigma <= 255.0)) return "min_sigma is outside 0 .. 255";
    if (!(o->amp >= 0.0 && std::isfinite(o->amp))) return "amp is negative or not finite";
    return nullptr;
}

hipError_t normalize_enqueue(hipStream_t st, const ccal_normalize_opts& o, int src_dtype, int dst_dtype, int width, int height, int n_img,
                             const void* src, void* dst) {
    NormArgs a = {};
    a.src = src; a.dst = dst;
    a.W = width; a.H = height; a.n_img = n_img;
    a.r = o.radius;
    const unsigned long long side = 2ull * (unsigned long long)o.radius + 1ull;
    a.n_win = side * side;
    a.floor_s = a.n_win * (unsigned long long)std::max(1.0, std::rint(257.0 * o.min_sigma));
    a.amp = o.amp;
    const int th = normalize_tile_h(o.radius);
    const TileGrid tg = tile_grid(width, height, kNormTileW, th, n_img);
    a.tiles_x = tg.tiles_x;
    const size_t lds = normalize_lds_bytes(o.radius);
    for_pix_type(src_dtype, [&](auto s) { for_pix_type(dst_dtype, [&](auto d) {
        using S = decltype(s); using D = decltype(d);
        switch (th) {
        case 32: hipLaunchKernelGGL((k_normalize<S, D, 32>), tg.grid, dim3(256), lds, st, a); break;
        case 16: hipLaunchKernelGGL((k_normalize<S, D, 16>), tg.grid, dim3(256), lds, st, a); break;
#ifdef CCAL_NORM_TILE_H
        default: hipLaunchKernelGGL((k_normalize<S, D, CCAL_NORM_TILE_H>), tg.grid, dim3(256), lds, st, a); break;
#endif
        }
    }); });
    return hipGetLastError();
}

}  // namespace

}  // namespace ccal

using namespace ccal;

extern "C" {

int ccal_normalize_set_defaults(ccal_normalize_opts* norm) {
    if (!norm) return CCAL_ERR_INVALID_ARG;
    norm->radius = 16; norm->reserved_ = 0;
    norm->min_sigma = 4.0; norm->amp = 64.0;
    return CCAL_OK;
}

int ccal_normalize_dev(ccal_ctx* ctx, int src_dtype, int dst_dtype, int width, int height, int n_img, const void* src_dev, void* dst_dev,
                       const ccal_normalize_opts* norm) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    const BadArg bad{ ctx, "ccal_normalize_dev" };
    if (!norm) return bad("norm is NULL");
    if (const char* what = normalize_check(norm)) return bad(what);
    const PairCheck pair = image_pair_check(src_dtype, dst_dtype, width, height, n_img, src_dev, dst_dev);
    if (!pair.go) return pair.what ? bad(pair.what) : CCAL_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, normalize_enqueue(ctx->stream, *norm, src_dtype, dst_dtype, width, height, n_img, src_dev, dst_dev));
    return CCAL_OK;
    CCAL_API_CATCH(ctx)
}

}  // extern "C"

// Grey frames from colour and raw Bayer frames, with binning (ccal_grey_dev), by the rule stated at the entry point in include/ccal.h:
// exact integers from the first term to the one rounding.  All images of a call in ONE launch:
//   k_grey<S, D, BIN, KIND>  a workgroup owns an output tile of 64 kx x th pixels of one image (grey_tile: kx and th from the bytes of a
//            source pixel and the bin, so that a tile row is at least 256 source bytes and the tile at most 32 KiB of LDS); blockIdx.x
//            walks the tiles of an image, blockIdx.y the images.  KIND: the channels of an interleaved pixel (1 = GREY, 3, 4), 0 = a
//            mosaic.  BGR(A) is RGB(A) with w_r and w_b swapped, the four mosaics differ in the parity of the R site: both are arguments.
//   tile     the BYTES of the tile's source rows go into LDS as they lie in memory (load_byte_rows of ccal_pix.hpp): 16-byte aligned
//            loads, one per lane, whatever the row's first byte - 3-byte pixels, odd widths, a block at any address; only a word that
//            reaches past an end of the caller's block falls back to its dwords.  No sample is loaded from global memory on its own.
//            A mosaic's tile has one more row above and below, reflected about the edge pixel at load time (the row is simply loaded
//            again), and one more column left and right where the image has one; a column beyond the image is reflected when read.
//   pixel    lane = an output pixel of a row; a wavefront takes the (row, 64-pixel group) items of the tile in turn.  The lane reads
//            its bin x bin source pixels (a mosaic: the (bin + 2)^2 samples around them) from LDS, sums each channel in 32 bits
//            (16 x 4 x 65535 < 2^22), then S = w_r R + w_g G + w_b B: 32 bits for a u8 source, whose samples stay on the 8-bit scale
//            (257 is a common factor: S = 257 S', S' < 2^30), 64 bits for a u16 source.
//   round    u8 -> u8: (S' + 2^(s-1)) >> s;  u8 -> u16: with S' = q 2^s + r, 257 q + ((257 r + 2^(s-1)) >> s), 257 r < 2^31;
//            u16 -> u16: (S + 2^(s-1)) >> s;  u16 -> u8: ((S + 257 2^(s-1)) >> s) / 257, a division of 32 bits by a constant.
//   stores   store_pixel_group: dwords of 4 u8 or 2 u16, pixel by pixel at the right edge and on unaligned rows.
// No atomics, no floating point: the unit needs no -ffp-contract line in csrc/Makefile.
#include <algorithm>
#include "ccal_call.hpp"
#include "ccal_pix.hpp"

namespace ccal {

constexpr int kGreyLdsBytes = 32768;

struct GreyArgs {
    const void* src;                   // [n_img][H][W][c]
    void* dst;                         // [n_img][Ho][Wo]
    unsigned long long src_bytes;      // of the whole source block
    int32_t W, H, Wo, Ho, n_img, tiles_x;
    int32_t kx_log2, th, stride;       // the tile is 64 kx x th output pixels, kx = 1, 2 or 4; the bytes between two tile rows in LDS
    int32_t rx, ry;                    // a mosaic: the parity of the R site's column and row
    uint32_t w_r, w_g, w_b;            // BGR(A): swapped
};

// the tile of a source pixel of `pxb` bytes at bin `bin`, with `halo` more rows and columns on every side
struct GreyTile { int kx_log2, th, stride; size_t lds; };
inline GreyTile grey_tile(int pxb, int bin, int halo, int Ho) {
    GreyTile g;
    const int row_bytes = 64 * bin * pxb;
    g.kx_log2 = row_bytes <= 64 ? 2 : row_bytes <= 128 ? 1 : 0;
    g.stride = byte_row_stride(((64 << g.kx_log2) * bin + 2 * halo) * pxb);
    g.th = std::max(1, std::min(32, (kGreyLdsBytes / g.stride - 2 * halo) / bin));
    if (g.th >= 4) g.th &= ~3;
    g.th = std::min(g.th, (Ho + 3) & ~3);
    g.lds = (size_t)(g.th * bin + 2 * halo) * (size_t)g.stride;
    return g;
}

template <class S> __device__ __forceinline__ unsigned grey_sample(const unsigned char* p) { return *reinterpret_cast<const S*>(p); }

template <class S, class D, int BIN, int KIND>
__global__ __launch_bounds__(256) void k_grey(const GreyArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_grey[];
    constexpr int C = KIND == 0 ? 1 : KIND, HALO = KIND == 0 ? 1 : 0, ES = (int)sizeof(S), PXB = C * ES;
    constexpr int SH = BIN == 1 ? 18 : BIN == 2 ? 20 : 22;                  // s = 18 + 2 log2(bin)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);              // said to be uniform: the rows' arithmetic below is scalar
    const int kx = 1 << a.kx_log2;
    const TileAt t = tile_at(a.tiles_x, 64 * kx, a.th);                     // the tile's first OUTPUT pixel: (t.x_t, t.y_t)
    const int xs0 = t.x_t * BIN, ys0 = t.y_t * BIN;                         // and its first source pixel
    const int rows_out = min(a.th, a.Ho - t.y_t);                           // output rows of this tile inside the image
    const int n_rows = rows_out * BIN + 2 * HALO;                           // tile row tt is source row ys0 - HALO + tt, reflected
    const int c_lo = max(xs0 - HALO, 0);                                    // the tile's source columns c_lo .. c_hi - 1, inside the image
    const int c_hi = min(min(xs0 + 64 * kx * BIN, a.Wo * BIN) + HALO, a.W);
    const int nb = (c_hi - c_lo) * PXB;
    const uintptr_t blk_lo = reinterpret_cast<uintptr_t>(a.src), blk_hi = blk_lo + a.src_bytes;
    D* dst = static_cast<D*>(a.dst);

    for (int img = blockIdx.y; img < a.n_img; img += gridDim.y) {
        auto row_addr = [&](int tt) -> uintptr_t {
            const int gy = HALO ? reflect_at_edge(ys0 - HALO + tt, a.H) : ys0 + tt;
            return blk_lo + (uintptr_t)((((int64_t)img * a.H + gy) * a.W + c_lo) * PXB);
        };
        // where tile row tt's first byte stands in its LDS row: the low four bits of row_addr(tt), which 32 bits give
        auto row_lds = [&](int tt) -> const unsigned char* {
            const int gy = HALO ? reflect_at_edge(ys0 - HALO + tt, a.H) : ys0 + tt;
            const unsigned low = (unsigned)blk_lo + (((unsigned)img * (unsigned)a.H + (unsigned)gy) * (unsigned)a.W + (unsigned)c_lo) * (unsigned)PXB;
            return lds_grey + tt * a.stride + (int)(low & 15u);
        };
        load_byte_rows(lds_grey, a.stride, n_rows, nb, blk_lo, blk_hi, tid, row_addr);
        __syncthreads();
        for (int it = wave; it < (rows_out << a.kx_log2); it += 4) {        // wave-uniform
            const int i = it >> a.kx_log2, g = it - (i << a.kx_log2);
            const int X = t.x_t + 64 * g + lane, Y = t.y_t + i;
            const int xs = min(X, a.Wo - 1) * BIN;                          // a lane beyond the right edge works on the last pixel and stores nothing
            unsigned sr = 0u, sg = 0u, sb = 0u;                             // the block's channel sums, a quarter of R4, G4, B4 each
            if constexpr (KIND != 0) {
#pragma unroll
                for (int dy = 0; dy < BIN; ++dy) {
                    const int tt = i * BIN + dy;
                    const unsigned char* p = row_lds(tt) + (xs - c_lo) * PXB;
#pragma unroll
                    for (int dx = 0; dx < BIN; ++dx) {
                        if constexpr (KIND == 1) sg += grey_sample<S>(p + dx * PXB);
                        else {
                            sr += grey_sample<S>(p + dx * PXB);
                            sg += grey_sample<S>(p + dx * PXB + ES);
                            sb += grey_sample<S>(p + dx * PXB + 2 * ES);
                        }
                    }
                }
                if constexpr (KIND == 1) { sr = sg; sb = sg; }
            } else {
                // the (BIN + 2)^2 samples around the block: column k is source column xs - 1 + k, reflected; row k tile row i BIN + k
                int co[BIN + 2];
#pragma unroll
                for (int k = 1; k <= BIN; ++k) co[k] = (xs - 1 + k - c_lo) * PXB;          // the block's own columns are inside the image
                co[0] = ((xs == 0 ? 1 : xs - 1) - c_lo) * PXB;                                // only its two neighbours can be beyond it
                co[BIN + 1] = ((xs + BIN >= a.W ? 2 * (a.W - 1) - (xs + BIN) : xs + BIN) - c_lo) * PXB;
                unsigned v[BIN + 2][BIN + 2];
#pragma unroll
                for (int k = 0; k < BIN + 2; ++k) {
                    const int tt = i * BIN + k;
                    const unsigned char* p = row_lds(tt);
#pragma unroll
                    for (int m = 0; m < BIN + 2; ++m) v[k][m] = grey_sample<S>(p + co[m]);
                }
                unsigned r4 = 0u, g4 = 0u, b4 = 0u;
#pragma unroll
                for (int dy = 0; dy < BIN; ++dy)
#pragma unroll
                    for (int dx = 0; dx < BIN; ++dx) {
                        const unsigned c4 = 4u * v[dy + 1][dx + 1];
                        const unsigned hor = v[dy + 1][dx] + v[dy + 1][dx + 2], ver = v[dy][dx + 1] + v[dy + 2][dx + 1];
                        const unsigned diag = v[dy][dx] + v[dy][dx + 2] + v[dy + 2][dx] + v[dy + 2][dx + 2];
                        const int px = ((xs + dx) & 1) ^ a.rx, py = ((Y * BIN + dy) & 1) ^ a.ry;   // (0,0) R, (1,1) B, (1,0) G in an R row, (0,1) G in a B row
                        const bool rb = px == py;
                        g4 += rb ? hor + ver : c4;
                        const unsigned first = rb ? c4 : 2u * hor, second = rb ? diag : 2u * ver;  // the site's own / its row's colour, and the other
                        const bool red_first = rb ? px == 0 : py == 0;
                        r4 += red_first ? first : second;
                        b4 += red_first ? second : first;
                    }
                sr = r4; sg = g4; sb = b4;                                   // four times the channel sums already
            }
            constexpr unsigned quad = KIND == 0 ? 1u : 4u;                 // the interleaved sums are a quarter of R4, G4, B4
            unsigned q;
            if constexpr (sizeof(S) == 1) {
                const unsigned s1 = (a.w_r * sr + a.w_g * sg + a.w_b * sb) * quad;      // S' < 2^30
                if constexpr (sizeof(D) == 1) q = (s1 + (1u << (SH - 1))) >> SH;
                else q = 257u * (s1 >> SH) + ((257u * (s1 & ((1u << SH) - 1u)) + (1u << (SH - 1))) >> SH);
            } else {
                const unsigned long long s2 = ((unsigned long long)a.w_r * sr + (unsigned long long)a.w_g * sg + (unsigned long long)a.w_b * sb) * quad;   // S < 2^38
                if constexpr (sizeof(D) == 2) q = (unsigned)((s2 + (1ull << (SH - 1))) >> SH);
                else q = (unsigned)((s2 + 257ull * (1ull << (SH - 1))) >> SH) / 257u;
            }
            store_pixel_group<D>(dst + ((int64_t)img * a.Ho + Y) * a.Wo, X, lane, a.Wo, q);
        }
        __syncthreads();                                                    // the next image's tile overwrites what the lanes read
    }
}

namespace {

template <class S, class D, int BIN>
void grey_launch_kind(int kind, dim3 grid, size_t lds, hipStream_t st, const GreyArgs& a) {
    switch (kind) {
    case 0: hipLaunchKernelGGL((k_grey<S, D, BIN, 0>), grid, dim3(256), lds, st, a); break;
    case 1: hipLaunchKernelGGL((k_grey<S, D, BIN, 1>), grid, dim3(256), lds, st, a); break;
    case 3: hipLaunchKernelGGL((k_grey<S, D, BIN, 3>), grid, dim3(256), lds, st, a); break;
    default: hipLaunchKernelGGL((k_grey<S, D, BIN, 4>), grid, dim3(256), lds, st, a); break;
    }
}

hipError_t grey_enqueue(hipStream_t st, const ccal_grey_opts& o, int layout, int src_dtype, int dst_dtype, int width, int height, int n_img,
                        const void* src, void* dst) {
    const bool bayer = layout_is_bayer(layout);
    const int kind = bayer ? 0 : layout_channels(layout);
    const int pxb = layout_channels(layout) * (src_dtype == CCAL_PIX_U16 ? 2 : 1);
    GreyArgs a = {};
    a.src = src; a.dst = dst;
    a.src_bytes = (unsigned long long)grey_src_image_bytes(layout, src_dtype, width, height) * (unsigned long long)n_img;
    a.W = width; a.H = height; a.Wo = width / o.bin; a.Ho = height / o.bin; a.n_img = n_img;
    const GreyTile g = grey_tile(pxb, o.bin, bayer ? 1 : 0, a.Ho);
    a.kx_log2 = g.kx_log2; a.th = g.th; a.stride = g.stride;
    const TileGrid tg = tile_grid(a.Wo, a.Ho, 64 << g.kx_log2, g.th, n_img);
    a.tiles_x = tg.tiles_x;
    a.rx = layout == CCAL_LAYOUT_BAYER_BGGR || layout == CCAL_LAYOUT_BAYER_GRBG;
    a.ry = layout == CCAL_LAYOUT_BAYER_BGGR || layout == CCAL_LAYOUT_BAYER_GBRG;
    const bool swap = layout == CCAL_LAYOUT_BGR || layout == CCAL_LAYOUT_BGRA;
    a.w_r = (uint32_t)(swap ? o.w_b : o.w_r); a.w_g = (uint32_t)o.w_g; a.w_b = (uint32_t)(swap ? o.w_r : o.w_b);
    for_pix_type(src_dtype, [&](auto s) { for_pix_type(dst_dtype, [&](auto d) {
        using S = decltype(s); using D = decltype(d);
        switch (o.bin) {
        case 1: grey_launch_kind<S, D, 1>(kind, tg.grid, g.lds, st, a); break;
        case 2: grey_launch_kind<S, D, 2>(kind, tg.grid, g.lds, st, a); break;
        default: grey_launch_kind<S, D, 4>(kind, tg.grid, g.lds, st, a); break;
        }
    }); });
    return hipGetLastError();
}

}  // namespace

}  // namespace ccal

using namespace ccal;

extern "C" {

int ccal_grey_set_defaults(ccal_grey_opts* opts) {
    if (!opts) return CCAL_ERR_INVALID_ARG;
    opts->bin = 1;
    opts->w_r = 19595; opts->w_g = 38470; opts->w_b = 7471;
    return CCAL_OK;
}

int ccal_grey_dev(ccal_ctx* ctx, int layout, int src_dtype, int dst_dtype, int width, int height, int n_img, const void* src_dev, void* dst_dev,
                  const ccal_grey_opts* opts) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    const BadArg bad{ ctx, "ccal_grey_dev" };
    const PairCheck pair = grey_stage_check(layout, src_dtype, dst_dtype, width, height, n_img, src_dev, dst_dev, opts);
    if (!pair.go) return pair.what ? bad(pair.what) : CCAL_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, grey_enqueue(ctx->stream, *opts, layout, src_dtype, dst_dtype, width, height, n_img, src_dev, dst_dev));
    return CCAL_OK;
    CCAL_API_CATCH(ctx)
}

}  // extern "C"

// What the image stages share about pixels: the table of the two pixel types, the quantisation, the load of a tile with its halo and
// the store of a wavefront's row of pixels (k_photo, k_normalize), the load of rows of bytes (k_grey, which stores as those two do), a
// workgroup's tile and the grid of tiles (those three and k_render),
// the run-time choice of the pixel type (every stage's launch).  Header only, every function forced inline: the code follows the
// -ffp-contract flag of the unit that includes it (off for render, photo and normalize, fast for the others - csrc/Makefile).
#pragma once
#include <algorithm>
#include <cstdint>
#include <hip/hip_runtime.h>
#include "../../include/ccal.h"

namespace ccal {

// hi: the largest value; scale: from the 0 .. 255 scale the stages compute on to the type's own; up: a pixel widened to 16 bits
template <class T> struct Pix;
template <> struct Pix<uint8_t> { static constexpr double hi = 255.0, scale = 1.0; static constexpr unsigned up = 257u; };
template <> struct Pix<uint16_t> { static constexpr double hi = 65535.0, scale = 257.0; static constexpr unsigned up = 1u; };

// Y on the 0 .. 255 scale -> the pixel: scaled, clamped, rounded half to even; 0 for a NaN
template <class D>
__device__ __forceinline__ unsigned pix_quantise(double Y) { return (unsigned)rint(fmin(fmax(Y * Pix<D>::scale, 0.0), Pix<D>::hi)); }

// the ih x iw tile from pixel (x_t - r, y_t - r) of the W x H image I, clamped to the image, into LDS as u16, by the 256 threads
template <class S>
__device__ __forceinline__ void load_halo_tile(uint16_t* tile_s, const S* I, int W, int H, int x_t, int y_t, int r, int iw, int ih, int tid) {
    for (int e = tid; e < ih * iw; e += 256) {
        const int ty = e / iw, tx = e - ty * iw;
        const int gx = min(max(x_t - r + tx, 0), W - 1), gy = min(max(y_t - r + ty, 0), H - 1);
        tile_s[e] = (uint16_t)((unsigned)I[(int64_t)gy * W + gx] * Pix<S>::up);
    }
}

// Rows of BYTES into LDS, for a stage whose pixels are not one sample each (k_grey: 3- and 4-channel pixels, mosaics with a reflected
// halo) and whose rows start on any byte: tile row t is the nb bytes from address row_addr(t) (0: the row is not wanted), and goes to
// lds + t * stride as the 16-byte-aligned words of global memory that cover it, one 16-byte load per lane - so byte b of the row
// stands at lds[t * stride + (row_addr(t) & 15) + b], and stride is a multiple of 16 of at least nb + 15 (byte_row_stride).  [lo, hi)
// is the caller's whole block: a word that reaches past either end of it is not loaded whole but as those of its four aligned dwords
// that hold at least one byte of the block (such a dword cannot cross a page), the others read as 0.  By the 256 threads.
__host__ __device__ constexpr int byte_row_stride(int nb) { return (nb + 15 + 15) & ~15; }
__device__ __forceinline__ uint4 load_word16_within(uintptr_t c, uintptr_t lo, uintptr_t hi) {
    typedef unsigned int word16 __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) word16* global_word16;   // the addresses are numbers: say that they are global ones,
    typedef const __attribute__((address_space(1))) uint32_t* global_word4;  // or the loads are flat ones
    if (c >= lo && c + 16 <= hi) {
        const word16 v = *(global_word16)c;
        return make_uint4(v.x, v.y, v.z, v.w);
    }
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uintptr_t d = c + 4u * (unsigned)k;
        w[k] = (d + 4 > lo && d < hi) ? *(global_word4)d : 0u;
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}
template <class RowAddr>
__device__ __forceinline__ void load_byte_rows(unsigned char* lds, int stride, int n_rows, int nb, uintptr_t lo, uintptr_t hi, int tid, RowAddr row_addr) {
    const int per_row = stride >> 4;
    for (int e = tid; e < n_rows * per_row; e += 256) {
        const int t = e / per_row, j = e - t * per_row;
        const uintptr_t a = row_addr(t);
        if (a == 0) continue;
        const uintptr_t c = (a & ~(uintptr_t)15) + 16u * (unsigned)j;
        if (c >= a + (unsigned)nb) continue;
        *reinterpret_cast<uint4*>(lds + t * stride + 16 * j) = load_word16_within(c, lo, hi);
    }
}
// a neighbour's coordinate reflected about the edge pixel of 0 .. n - 1 (n >= 2, i in -1 .. n): a mosaic keeps its parity
__host__ __device__ __forceinline__ int reflect_at_edge(int i, int n) { return i < 0 ? -i : i >= n ? 2 * (n - 1) - i : i; }

// The store of a wavefront's row of quantised pixels, lane `lane` holding the value q of pixel x of `row` (W pixels): the lanes of a
// group of 4 (u8) or 2 (u16) adjacent pixels hand their pixels to the group's first lane, which stores them as one dword; a group that
// ends at the image's right edge, or whose first pixel is not on a dword boundary (a width that is no multiple of 4 bytes), stores pixel by
// pixel: no lane ever writes a byte outside the image.  Every lane of the wavefront must be here (the shuffle); those with x >= W store nothing.
template <class D>
__device__ __forceinline__ void store_pixel_group(D* row, int x, int lane, int W, unsigned q) {
    constexpr int PX = 4 / (int)sizeof(D), BITS = 8 * (int)sizeof(D);
    unsigned word = q;
#pragma unroll
    for (int k = 1; k < PX; ++k) word |= (unsigned)__shfl_down((int)q, k, 64) << (BITS * k);
    const int x_g = x - (lane & (PX - 1));                         // the group's first pixel
    const bool whole = x_g + PX <= W && (reinterpret_cast<uintptr_t>(row + x_g) & 3u) == 0;
    if (whole) {
        if ((lane & (PX - 1)) == 0) *reinterpret_cast<uint32_t*>(row + x) = word;
    } else if (x < W) row[x] = (D)q;
}

// blockIdx.x walks an image's tiles of tw x th pixels row by row, blockIdx.y the images, in a loop where there are more than 65535:
// the workgroup's tile and its first pixel, and the launch's grid with the tiles in a row, which the kernel's arguments carry
struct TileAt { int tile_x, tile_y, x_t, y_t; };
__device__ __forceinline__ TileAt tile_at(int tiles_x, int tw, int th) {
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    return { tile_x, tile_y, tile_x * tw, tile_y * th };
}
struct TileGrid { int tiles_x; dim3 grid; };
inline TileGrid tile_grid(int W, int H, int tw, int th, int n_img) {
    const int tiles_x = (W + tw - 1) / tw, tiles_y = (H + th - 1) / th;
    return { tiles_x, dim3((unsigned)(tiles_x * tiles_y), (unsigned)std::min(n_img, 65535)) };
}

// f(uint16_t{}) or f(uint8_t{}) by a checked ccal_pixel_type: f is a generic lambda that launches the kernel of decltype of its argument
template <class F> void for_pix_type(int dtype, F&& f) { if (dtype == CCAL_PIX_U16) f(uint16_t{}); else f(uint8_t{}); }

}  // namespace ccal

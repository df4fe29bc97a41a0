// The store of a wavefront's row of quantised pixels, shared by the image kernels whose lane l holds pixel x of a row (k_photo,
// k_normalize): the lanes of a group of 4 (u8) or 2 (u16) adjacent pixels hand their pixels to the group's first lane, which stores
// them as one dword; a group that ends at the image's right edge, or whose first pixel is not on a dword boundary (rows of a width
// that is no multiple of 4 bytes), stores pixel by pixel: no lane ever writes a byte outside the image.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace ccal {

// `row`: the first pixel of the image row, W pixels wide; lane `lane` holds the value q of pixel x = (the wavefront's first pixel) +
// lane.  Every lane of the wavefront must be here (the shuffle), the lanes with x >= W included; they store nothing.
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

}  // namespace ccal

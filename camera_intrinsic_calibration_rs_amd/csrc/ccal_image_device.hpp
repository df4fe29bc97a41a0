// What the kernels of the image stages share (ccal_kernels_detect / corners / quads / tags / tagchain / board.hip): the f64 bilinear sample,
// the row-to-image search over CSR offsets and an image's clamped span of them, the hand-off between lanes of one wavefront and the wavefront's int32 scan.  Header only,
// every function forced inline: the code follows the flags of the unit that includes it (-ffp-contract=off for quads, tags and board, fast
// for the others - csrc/Makefile), so there is no translation unit of its own.  The choice of a launch's pixel type: ccal_pix.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include "ccal_pix.hpp"

namespace ccal {

// producer and consumer are lanes of the same wavefront: its LDS and memory operations execute in order, this only keeps the compiler
// from moving accesses across the hand-off
__device__ __forceinline__ void wave_handoff() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the inclusive scan of v over the 64 lanes of a wavefront; lane = the caller's lane number
__device__ __forceinline__ int32_t wave_scan_inclusive(int32_t v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// the image that owns row g of a CSR batch: the last k < n_img with off[k] <= g (images without rows are stepped over)
__device__ __forceinline__ int image_of_row(const int64_t* off, int n_img, int64_t g) {
    int lo = 0, hi = n_img;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// the rows of image k of a CSR batch that a walk may visit: off[k + 1] - off[k], clamped to 0 .. cap, the size its arrays were given
__device__ __forceinline__ int csr_span(const int64_t* off, int k, int cap) {
    const int64_t m = off[k + 1] - off[k];
    return (int)(m < 0 ? 0 : (m > (int64_t)cap ? (int64_t)cap : m));
}

// floor and fraction of one coordinate, the two neighbour indices clamped to [0, n - 1]
__device__ __forceinline__ void image_tap(double x, int32_t n, int32_t& i0, int32_t& i1, double& ax) {
    const double f = floor(x);
    ax = x - f;
    const double hi = (double)(n - 1);
    i0 = (int32_t)fmin(fmax(f, 0.0), hi);            // NaN: fmax gives 0
    i1 = min(i0 + 1, n - 1);
}

// the bilinear f64 sample of a W x H image at (x, y)
template <class T>
__device__ __forceinline__ double image_sample(const T* img, int32_t W, int32_t H, double x, double y) {
    int32_t x0, x1, y0, y1;
    double ax, ay;
    image_tap(x, W, x0, x1, ax);
    image_tap(y, H, y0, y1, ay);
    const T* r0 = img + (int64_t)y0 * W;
    const T* r1 = img + (int64_t)y1 * W;
    const double p00 = (double)r0[x0], p01 = (double)r0[x1], p10 = (double)r1[x0], p11 = (double)r1[x1];
    // the difference form: a constant neighbourhood samples to exactly its value, whatever the fractions
    const double top = p00 + ax * (p01 - p00), bot = p10 + ax * (p11 - p10);
    return top + ay * (bot - top);
}

}  // namespace ccal

// Checkerboard-corner candidates of whole images (ccal_detect_corners_batch / _dev): the integer saddle rule stated at the entry
// points in include/ccal.h - binomial smoothing, the Hessian at step s, R = hxy^2 - 16 hxx hyy, non-maximum suppression in a
// (2r+1)^2 window, a threshold relative to the image's largest R.  Integers only; tests/detect_ref.py is met bit for bit.
//   k_detect_tiles  ONE pass over the images.  A workgroup owns a 32 x 32 tile of the domain of one image.  It stages the tile
//                   plus its halo (r + s + 2 on every side) in LDS as u16, smooths it there separably (rows, then columns, int32),
//                   forms R (int64) over the tile plus r, and tests its own 1 024 pixels against their windows.  The local-maximum
//                   test does not depend on the threshold, so every local maximum with R >= min_response is kept, and the
//                   threshold is applied afterwards.  Two local maxima are never within r of each other in both coordinates (the
//                   tie rule), so each (r+1) x (r+1) block of the domain holds at most one: a maximum is written to the SLOT of its
//                   block - no counter, no arrival order.  The tile's largest R goes into the image's Rmax by an integer atomicMax.
//   k_detect_rows   one workgroup per image: T from Rmax, then per domain row the number of kept slots with R >= T (a thread
//                   walks the slots of its row's block row), an exclusive scan over the rows, the image's count.
//   k_detect_emit   one thread per domain row walks the same slots again and writes its candidates, in x order, at the row's
//                   offset: row-major order of (y, x) by construction.  Candidates past cap are counted, not stored.
// No per-pixel response map leaves the LDS.  Every global index is guarded by the image / slot / row bounds it was sized with.
#include <algorithm>
#include <cstring>
#include <vector>
#include "ccal_chain_front.hpp"
#include "ccal_image_device.hpp"

namespace ccal {

constexpr int kDetTile = 32;                  // the tile's side in domain pixels
constexpr int kDetThreads = 256;
constexpr int kDetMaxStep = 4, kDetMaxRadius = 15;
constexpr int64_t kDetNone = INT64_MIN;       // R of a pixel outside the domain: it never competes

// DetectArgs: ccal_internal.hpp

__host__ __device__ inline size_t det_up16(size_t b) { return (b + 15) & ~(size_t)15; }
// LDS of k_detect_tiles: S [SW][SW] int32 | a union of { Hs [IW][SW] int32, I [IW][IW] u16 } and R [RW][RW] int64
inline size_t det_lds_bytes(int s, int r) {
    const size_t RW = kDetTile + 2 * r, SW = RW + 2 * s, IW = SW + 4;
    return det_up16(SW * SW * 4) + std::max(RW * RW * 8, det_up16(IW * SW * 4) + IW * IW * 2);
}

// T of an image; INT64_MAX: no candidate (Rmax <= 0)
__device__ __forceinline__ int64_t det_threshold(long long rmax, int64_t min_response, int32_t rel_q10) {
    if (rmax <= 0) return INT64_MAX;
    const int64_t t = (int64_t)(rmax >> 10) * (int64_t)rel_q10;
    return t > min_response ? t : min_response;
}

// a lane's walk over the positions tid, tid + kDetThreads, ... of a region w wide: (x, y) by increments, two divisions per walk
// instead of one per element (kDetThreads mod w < w, so one wrap per step is enough)
struct DetWalk {
    int x, y, dx, dy, w;
    __device__ __forceinline__ DetWalk(int tid, int w_) : w(w_) { y = tid / w; x = tid - y * w; dy = kDetThreads / w; dx = kDetThreads - dy * w; }
    __device__ __forceinline__ void next() { x += dx; y += dy; if (x >= w) { x -= w; ++y; } }
};

template <class T>
__global__ __launch_bounds__(kDetThreads) void k_detect_tiles(const DetectArgs a) {
    extern __shared__ __align__(16) unsigned char det_lds[];
    const int s = a.s, r = a.r, W = a.W, H = a.H;
    const int RW = kDetTile + 2 * r, SW = RW + 2 * s, IW = SW + 4;
    int32_t* S = reinterpret_cast<int32_t*>(det_lds);
    unsigned char* U = det_lds + det_up16((size_t)SW * SW * 4);
    int32_t* Hs = reinterpret_cast<int32_t*>(U);
    uint16_t* I = reinterpret_cast<uint16_t*>(U + det_up16((size_t)IW * SW * 4));
    int64_t* R = reinterpret_cast<int64_t*>(U);
    const int tid = threadIdx.x, k = blockIdx.z;
    const int ox = a.d0 + kDetTile * (int)blockIdx.x, oy = a.d0 + kDetTile * (int)blockIdx.y;     // the tile's first pixel
    const int ix0 = ox - r - s - 2, iy0 = oy - r - s - 2;                                          // the staged region's
    const T* img = static_cast<const T*>(a.img) + (int64_t)k * W * H;
    const int x_hi = a.d0 + a.dw, y_hi = a.d0 + a.dh;                                              // one past the domain

    // stage: every pixel of the region once, 0 outside the image (such a pixel feeds only S of pixels outside the domain)
    DetWalk wi(tid, IW);
    for (int p = tid; p < IW * IW; p += kDetThreads, wi.next()) {
        const int gx = ix0 + wi.x, gy = iy0 + wi.y;
        const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
        I[p] = in ? (uint16_t)img[(int64_t)gy * W + gx] : (uint16_t)0;
    }
    __syncthreads();
    // rows: Hs(x, y) = sum b(i) I(x + i, y) for the SW columns from ix0 + 2, all IW rows
    DetWalk wh(tid, SW);
    for (int p = tid; p < IW * SW; p += kDetThreads, wh.next()) {
        const uint16_t* q = I + wh.y * IW + wh.x;
        Hs[p] = (int32_t)q[0] + 4 * (int32_t)q[1] + 6 * (int32_t)q[2] + 4 * (int32_t)q[3] + (int32_t)q[4];
    }
    __syncthreads();
    // columns: S over the SW x SW pixels from (ix0 + 2, iy0 + 2) = (ox - r - s, oy - r - s)
    for (int p = tid; p < SW * SW; p += kDetThreads) {       // position p of S reads position p of Hs and the four rows below
        const int32_t* q = Hs + p;
        S[p] = q[0] + 4 * q[SW] + 6 * q[2 * SW] + 4 * q[3 * SW] + q[4 * SW];
    }
    __syncthreads();                                  // Hs and I are dead: R takes their place
    DetWalk wr(tid, RW);
    for (int p = tid; p < RW * RW; p += kDetThreads, wr.next()) {
        const int x = wr.x, y = wr.y, gx = ox - r + x, gy = oy - r + y;
        int64_t v = kDetNone;
        if (gx >= a.d0 && gx < x_hi && gy >= a.d0 && gy < y_hi) {
            const int32_t* c = S + (y + s) * SW + (x + s);
            const int32_t c0 = c[0];
            const int64_t hxx = c[s] - 2 * c0 + c[-s], hyy = c[s * SW] - 2 * c0 + c[-s * SW];
            const int64_t hxy = c[s * SW + s] - c[-s * SW + s] - c[s * SW - s] + c[-s * SW - s];
            v = hxy * hxy - 16 * hxx * hyy;
        }
        R[p] = v;
    }
    __syncthreads();

    long long best = 0;
    const int tx = tid & (kDetTile - 1);
    for (int ty = tid / kDetTile; ty < kDetTile; ty += kDetThreads / kDetTile) {
        const int gx = ox + tx, gy = oy + ty;
        if (gx >= x_hi || gy >= y_hi) continue;
        const int64_t* c = R + (ty + r) * RW + (tx + r);
        const int64_t rp = c[0];
        best = rp > best ? rp : best;
        if (rp < a.min_response) continue;
        bool ok = true;
        for (int dy = -r; dy <= r && ok; ++dy) {
            const int64_t* row = c + dy * RW;
            for (int dx = -r; dx <= r; ++dx) {
                const int64_t q = row[dx];
                const bool before = dy < 0 || (dy == 0 && dx < 0);
                ok = ok && (before ? rp > q : rp >= q);
            }
        }
        if (!ok) continue;
        const int bx = (gx - a.d0) / (r + 1), by = (gy - a.d0) / (r + 1);
        if (bx >= a.nbx || by >= a.nby) continue;     // cannot happen: the slot arrays were sized from the same domain
        const int64_t slot = (int64_t)k * a.nbx * a.nby + (int64_t)by * a.nbx + bx;
        const int32_t* cs = S + (ty + r + s) * SW + (tx + r + s);
        const int32_t c0 = cs[0];
        a.hess[3 * slot + 0] = cs[s] - 2 * c0 + cs[-s];
        a.hess[3 * slot + 1] = cs[s * SW] - 2 * c0 + cs[-s * SW];
        a.hess[3 * slot + 2] = cs[s * SW + s] - cs[-s * SW + s] - cs[s * SW - s] + cs[-s * SW - s];
        a.resp[slot] = rp;
        a.pix[slot] = gy * W + gx;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const long long o = __shfl_xor(best, off, 64);
        best = o > best ? o : best;
    }
    if ((tid & 63) == 0 && best > 0) atomicMax(a.rmax + k, best);
}

// the kept slots of domain row `row` of image k with R >= T, in x order: f(slot) for each
template <class F>
__device__ __forceinline__ void det_row_slots(const DetectArgs& a, int k, int row, int64_t T, F f) {
    const int by = row / (a.r + 1);
    const int32_t lo = (a.d0 + row) * a.W, hi = lo + a.W;     // pix of that image row: lo <= pix < hi (at most 2^31 - 1 pixels)
    const int64_t base = (int64_t)k * a.nbx * a.nby + (int64_t)by * a.nbx;
    for (int bx = 0; bx < a.nbx; ++bx) {
        const int32_t p = a.pix[base + bx];
        if (p >= lo && p < hi && a.resp[base + bx] >= T) f(base + bx, p - lo);
    }
}

__global__ __launch_bounds__(kDetThreads) void k_detect_rows(const DetectArgs a) {
    __shared__ int32_t wave_sum[kDetThreads / 64];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t T = det_threshold(a.rmax[k], a.min_response, a.rel_q10);
    int32_t carry = 0;
    for (int base = 0; base < a.dh; base += kDetThreads) {
        const int row = base + tid;
        int32_t c = 0;
        if (row < a.dh && T != INT64_MAX) det_row_slots(a, k, row, T, [&](int64_t, int32_t) { ++c; });
        const int32_t inc = wave_scan_inclusive(c, lane);
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        int32_t front = 0, total = 0;
        for (int w = 0; w < kDetThreads / 64; ++w) { if (w < wave) front += wave_sum[w]; total += wave_sum[w]; }
        if (row < a.dh) a.rowoff[(int64_t)k * a.dh + row] = carry + front + inc - c;
        carry += total;
        __syncthreads();                               // wave_sum is rewritten by the next round
    }
    if (tid == 0) a.count[k] = carry;
}

__global__ __launch_bounds__(kDetThreads) void k_detect_emit(const DetectArgs a) {
    const int k = blockIdx.y, row = blockIdx.x * kDetThreads + threadIdx.x;
    if (row >= a.dh) return;
    const int64_t T = det_threshold(a.rmax[k], a.min_response, a.rel_q10);
    if (T == INT64_MAX) return;
    int32_t rank = a.rowoff[(int64_t)k * a.dh + row];
    const int64_t out0 = a.imgoff[k], room = a.imgoff[k + 1] - out0;        // room = min(count, cap)
    det_row_slots(a, k, row, T, [&](int64_t slot, int32_t x) {
        if (rank >= 0 && rank < a.cap && rank < room) {
            const int64_t o = out0 + rank;
            a.oxy[2 * o] = x; a.oxy[2 * o + 1] = a.d0 + row;
            a.ohess[3 * o] = a.hess[3 * slot]; a.ohess[3 * o + 1] = a.hess[3 * slot + 1]; a.ohess[3 * o + 2] = a.hess[3 * slot + 2];
            a.oresp[o] = a.resp[slot];
        }
        ++rank;
    });
}

const char* detect_bad_params(int step, int nms_radius, int64_t min_response, int rel_q10, int cap) {
    if (step < 1 || step > kDetMaxStep) return "step outside 1 .. 4";
    if (nms_radius < 1 || nms_radius > kDetMaxRadius) return "nms_radius outside 1 .. 15";
    if (min_response < 1) return "min_response < 1";
    if (rel_q10 < 0 || rel_q10 > 1024) return "rel_q10 outside 0 .. 1024";
    if (cap < 1) return "cap < 1";
    return nullptr;
}

hipError_t detect_enqueue_find(hipStream_t s, int dtype, const DetectArgs& a) {
    const size_t nb = (size_t)a.nbx * (size_t)a.nby, m = (size_t)a.n;
    hipError_t e = hipMemsetAsync(a.pix, 0xFF, nb * m * sizeof(int32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(a.rmax, 0, m * sizeof(long long), s);
    if (e != hipSuccess) return e;
    const size_t lds = det_lds_bytes(a.s, a.r);
    const dim3 grid((unsigned)((a.dw + kDetTile - 1) / kDetTile), (unsigned)((a.dh + kDetTile - 1) / kDetTile), (unsigned)m);
    for_pix_type(dtype, [&](auto t) { hipLaunchKernelGGL(k_detect_tiles<decltype(t)>, grid, dim3(kDetThreads), lds, s, a); });
    hipLaunchKernelGGL(k_detect_rows, dim3((unsigned)m), dim3(kDetThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t detect_enqueue_emit(hipStream_t s, const DetectArgs& a) {
    hipLaunchKernelGGL(k_detect_emit, dim3((unsigned)((a.dh + kDetThreads - 1) / kDetThreads), (unsigned)a.n), dim3(kDetThreads), 0, s, a);
    return hipGetLastError();
}

namespace {

int detect_call(ccal_ctx* ctx, const char* where, const GreyBatch& b, int step, int nms_radius, int64_t min_response, int rel_q10, int cap,
                int32_t* count_out, int32_t* xy_out, int32_t* hess_out, int64_t* response_out) {
    const BadArg bad{ ctx, where };
    if (const char* what = detect_bad_params(step, nms_radius, min_response, rel_q10, cap)) return bad(what);
    if (const char* what = b.bad()) return bad(what);
    const int n_img = b.n_img;
    if (n_img == 0) return CCAL_OK;
    if (!b.images || !count_out || !xy_out || !hess_out) return bad("NULL argument");

    const DetectDomain dm = detect_domain(b.width, b.height, step, nms_radius);
    if (!dm.dw) {                                      // no domain: nothing to launch
        std::fill(count_out, count_out + n_img, 0);
        return CCAL_OK;
    }
    const size_t nb = dm.slots(), dh = (size_t)dm.dh, rows_cap = std::min<size_t>((size_t)cap, nb);
    const size_t per_image = nb * 24 + dh * 4 + rows_cap * 24 + b.staged_bytes(1) + 64;
    const size_t nc = chain_images_per_chunk((size_t)n_img, per_image, test_chunk_bytes("CCAL_TEST_DETECT_CHUNK_BYTES", kChainChunkBytes));

    // one block for the largest chunk: images (host call) | slots | rows, counts, offsets | the stored rows
    CallBlock blk(ctx);
    DetectSlices sl;
    sl.add(blk, b, dm, rows_cap, nc);
    if (!blk.alloc()) return blk.finish(where);

    DetectArgs a = sl.args(blk, b, dm, step, nms_radius, min_response, rel_q10, cap);
    std::vector<int64_t> imgoff(nc + 1);
    std::vector<int32_t> h_xy, h_hess;
    std::vector<int64_t> h_resp;

    for (size_t k0 = 0; k0 < (size_t)n_img && blk.ok(); k0 += nc) {
        const size_t m = std::min(nc, (size_t)n_img - k0);
        a.n = (int32_t)m;
        blk.poison(sl.hess, sl.resp);                  // the test hook's 0xFF over what the kernels write before they read it:
        blk.poison(sl.oxy, sl.oresp);                  // the slots' payload and the stored rows (not the indices, counts and offsets)
        a.img = b.chunk(blk, sl.img, k0, m);
        if (blk.ok()) blk.note(detect_enqueue_find(ctx->stream, b.dtype, a));
        blk.download(count_out + k0, a.count, m);
        if (blk.ok()) blk.note(hipStreamSynchronize(ctx->stream));
        if (!blk.ok()) break;
        imgoff[0] = 0;
        for (size_t i = 0; i < m; ++i) imgoff[i + 1] = imgoff[i] + std::min<int64_t>(count_out[k0 + i], (int64_t)rows_cap);
        const size_t total = (size_t)imgoff[m];
        if (!total) continue;
        blk.upload(sl.imgoff, imgoff.data(), m + 1);
        if (blk.ok()) blk.note(detect_enqueue_emit(ctx->stream, a));
        h_xy.resize(2 * total); h_hess.resize(3 * total);
        if (response_out) h_resp.resize(total);
        blk.download(h_xy.data(), a.oxy, 2 * total);
        blk.download(h_hess.data(), a.ohess, 3 * total);
        blk.download(response_out ? h_resp.data() : nullptr, a.oresp, total);
        if (blk.ok()) blk.note(hipStreamSynchronize(ctx->stream));
        if (!blk.ok()) break;
        for (size_t i = 0; i < m; ++i) {               // the chunk's rows, image after image, to [k][cap] of the caller's arrays
            const size_t at = (size_t)imgoff[i], rows = (size_t)(imgoff[i + 1] - imgoff[i]), k = k0 + i;
            if (!rows) continue;
            std::memcpy(xy_out + 2 * k * (size_t)cap, h_xy.data() + 2 * at, rows * 2 * sizeof(int32_t));
            std::memcpy(hess_out + 3 * k * (size_t)cap, h_hess.data() + 3 * at, rows * 3 * sizeof(int32_t));
            if (response_out) std::memcpy(response_out + k * (size_t)cap, h_resp.data() + at, rows * sizeof(int64_t));
        }
    }
    return blk.finish(where);
}

}  // namespace
}  // namespace ccal

using namespace ccal;

extern "C" {

int ccal_detect_corners_batch(ccal_ctx* ctx, int dtype, int width, int height, int n_img, const void* images, int step, int nms_radius,
                              int64_t min_response, int rel_q10, int cap, int32_t* count_out, int32_t* xy_out, int32_t* hess_out,
                              int64_t* response_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    return detect_call(ctx, "ccal_detect_corners_batch", GreyBatch{ dtype, width, height, n_img, images, false }, step, nms_radius, min_response,
                       rel_q10, cap, count_out, xy_out, hess_out, response_out);
    CCAL_API_CATCH(ctx)
}

int ccal_detect_corners_dev(ccal_ctx* ctx, int dtype, int width, int height, int n_img, const void* images_dev, int step, int nms_radius,
                            int64_t min_response, int rel_q10, int cap, int32_t* count_out, int32_t* xy_out, int32_t* hess_out,
                            int64_t* response_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    return detect_call(ctx, "ccal_detect_corners_dev", GreyBatch{ dtype, width, height, n_img, images_dev, true }, step, nms_radius, min_response,
                       rel_q10, cap, count_out, xy_out, hess_out, response_out);
    CCAL_API_CATCH(ctx)
}

}  // extern "C"

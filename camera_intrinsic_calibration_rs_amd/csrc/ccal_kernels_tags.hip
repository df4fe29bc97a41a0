// Tag decoding (ccal_decode_tags_batch / _dev): every candidate quad of a batch of grey images sampled on the tag's cell grid and
// matched against a caller-supplied code table, by the rule stated at the entry points in include/ccal.h.  All quads of a chunk of
// images in ONE launch, one wavefront per quad, four per workgroup:
//   cells    lane l owns the cells l, l + 64, l + 128 of the n x n grid (n <= 12: at most 144 cells, three per lane): the quad's
//            projective map, S x S bilinear f64 samples per cell, their mean - in registers, nothing goes through LDS
//   decide   lo / hi / margin by a min / max butterfly (exact, order-free); the white cells of each 64-cell chunk as one __ballot
//            mask; the border count from the masks; the data bits of the four turns by four more ballots (lane l supplies the bit
//            of weight 2^l, so at d = 8 the code fills the 64 lanes and no shift by 64 occurs)
//   match    the family is staged in LDS by the whole workgroup, kTagFamChunk codes at a time; lane l tests the codes l, l + 64, ..
//            of the chunk against the four turns and keeps the smallest key (hamming << 40 | m << 2 | k); one xor butterfly of
//            that integer leaves the rule's lexicographic minimum on every lane
// The wavefronts of a workgroup meet only at the barriers around the family's staging, and every wavefront reaches every one of
// them: a wavefront without a quad, or whose quad is already decided, still walks the chunks.  No atomics; the lane-to-cell and
// lane-to-code mappings are fixed, so a quad's outputs are a pure function of its image, its corners, the family and the parameters.
// This unit is compiled with -ffp-contract=off (csrc/Makefile): the outputs are decisions, and tests/tag_ref.py, the numpy f64
// yardstick, rounds every product and sum on its own.  Every pixel index is clamped to the image; the inside test makes the clamp a
// no-op, the clamp stays as the guard.
#include <algorithm>
#include <cmath>
#include <vector>
#include "ccal_call.hpp"
#include "ccal_image_device.hpp"
#include "ccal_image_plan.hpp"

namespace ccal {

constexpr int kTagWaves = 4;                  // wavefronts (= quads in flight) per workgroup
constexpr int kTagMaxSide = 12;               // n = d + 2 border <= 12: at most 144 cells
constexpr int kTagCellChunks = 3;             // cells per lane
constexpr int kTagFamChunk = 512;             // codes staged at a time: 4 KB of LDS
constexpr size_t kTagChunkBytes = (size_t)256 << 20;      // the block one launch should need: larger batches go image chunk by chunk

// TagArgs: ccal_internal.hpp

__device__ __forceinline__ double tag_wave_min(double v) {
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ double tag_wave_max(double v) {
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

template <class T>
__global__ __launch_bounds__(64 * kTagWaves) void k_decode_tags(const TagArgs a) {
    __shared__ unsigned long long fam[kTagFamChunk];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * kTagWaves + wave;
    const bool have = g < a.n;                           // wave-uniform; a wavefront without a quad only helps to stage the family
    const int d = a.d, n = a.d + 2 * a.border, nn = n * n, dd = a.d * a.d, S = a.S;
    const int32_t W = a.W, H = a.H;

    int reason = CCAL_TAG_OUTSIDE;
    double margin = __builtin_nan("");
    unsigned long long code[4] = { 0, 0, 0, 0 };
    double qx[4] = { 0, 0, 0, 0 }, qy[4] = { 0, 0, 0, 0 };
    bool matching = false;                               // wave-uniform: the quad has passed the border test

    if (have) {
        const T* img = static_cast<const T*>(a.img) + (int64_t)image_of_row(a.off, a.n_img, a.q0 + g) * W * H;
        for (int i = 0; i < 4; ++i) { qx[i] = a.quads[8 * g + 2 * i]; qy[i] = a.quads[8 * g + 2 * i + 1]; }

        // 1. the map of the unit square onto the quad
        const double sx = qx[0] - qx[1] + qx[2] - qx[3], sy = qy[0] - qy[1] + qy[2] - qy[3];
        const double d1x = qx[1] - qx[2], d1y = qy[1] - qy[2], d2x = qx[3] - qx[2], d2y = qy[3] - qy[2];
        const double den = d1x * d2y - d2x * d1y;
        const double mg = (sx * d2y - d2x * sy) / den, mh = (d1x * sy - sx * d1y) / den;
        const double ma = qx[1] - qx[0] + mg * qx[1], mb = qx[3] - qx[0] + mh * qx[3], mc = qx[0];
        const double md = qy[1] - qy[0] + mg * qy[1], me = qy[3] - qy[0] + mh * qy[3], mf = qy[0];
        const double x_hi = (double)(W - 1), y_hi = (double)(H - 1), dn = (double)n, s2 = (double)(2 * S), ss = (double)(S * S);

        // 2., 3. the lane's cells: S x S samples each, every sample point inside the image
        double val[kTagCellChunks];
        bool inside = true;
#pragma unroll
        for (int ch = 0; ch < kTagCellChunks; ++ch) {
            const int cell = lane + 64 * ch;
            val[ch] = 0.0;
            if (cell < nn) {
                const int cj = cell / n, ci = cell - cj * n;
                double acc = 0.0;
                for (int q = 0; q < S; ++q) {
                    const double v = ((double)cj + (double)(2 * q + 1) / s2) / dn;
                    for (int p = 0; p < S; ++p) {
                        const double u = ((double)ci + (double)(2 * p + 1) / s2) / dn;
                        const double w = mg * u + mh * v + 1.0;
                        const double x = (ma * u + mb * v + mc) / w, y = (md * u + me * v + mf) / w;
                        // false for NaN; +-inf fail one of the two sides
                        const bool ok = w > 0.0 && w <= 1.79769313486231570815e308 && x >= 0.0 && x <= x_hi && y >= 0.0 && y <= y_hi;
                        inside = inside && ok;
                        if (ok) acc += image_sample(img, W, H, x, y);
                    }
                }
                val[ch] = acc / ss;
            }
        }

        if (__all(inside)) {
            // 4. threshold
            double vmin = __builtin_inf(), vmax = -__builtin_inf();
#pragma unroll
            for (int ch = 0; ch < kTagCellChunks; ++ch)
                if (lane + 64 * ch < nn) { vmin = fmin(vmin, val[ch]); vmax = fmax(vmax, val[ch]); }
            const double lo = tag_wave_min(vmin), hi = tag_wave_max(vmax);
            const double t = lo + (hi - lo) / 2.0;
            double mm = __builtin_inf();
            unsigned long long mask[kTagCellChunks];
            int border_white = 0;
#pragma unroll
            for (int ch = 0; ch < kTagCellChunks; ++ch) {
                const int cell = lane + 64 * ch;
                const bool live = cell < nn;
                if (live) mm = fmin(mm, fabs(val[ch] - t));
                const bool white = live && val[ch] > t;
                const int cj = cell / n, ci = cell - cj * n;
                const bool data = ci >= a.border && ci < a.border + d && cj >= a.border && cj < a.border + d;
                mask[ch] = __ballot(white);
                border_white += __popcll(__ballot(white && !data));
            }
            margin = tag_wave_min(mm);
            if (!(hi - lo >= a.min_contrast)) reason = CCAL_TAG_LOW_CONTRAST;
            else {
                // 6., 7. lane l supplies the bit of weight 2^l: data cell number dd - 1 - l in row-major order, seen through k turns
                const int idx = dd - 1 - lane;
                int r = idx / d, c = idx - r * d;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    bool bit = false;
                    if (lane < dd) {
                        const int cell = (a.border + r) * n + a.border + c;
                        const unsigned long long m = cell < 64 ? mask[0] : (cell < 128 ? mask[1] : mask[2]);
                        bit = (m >> (cell & 63)) & 1ull;
                    }
                    code[k] = __ballot(bit);
                    const int r1 = d - 1 - c;            // T(B)(r, c) = B(d - 1 - c, r)
                    c = r; r = r1;
                }
                // 5. border
                if (border_white > a.max_border) reason = CCAL_TAG_BORDER;
                else { reason = CCAL_TAG_NO_CODE; matching = true; }
            }
        }
    }

    // 8. the smallest (hamming, m, k) over the family, staged kTagFamChunk codes at a time by the whole workgroup
    unsigned long long best = ~0ull;
    for (int base = 0; base < a.n_codes; base += kTagFamChunk) {
        const int cnt = min(kTagFamChunk, a.n_codes - base);
        __syncthreads();                                 // the chunk before this one has been read by every wavefront
        for (int i = threadIdx.x; i < cnt; i += 64 * kTagWaves) fam[i] = a.codes[base + i];
        __syncthreads();
        if (matching)
            for (int i = lane; i < cnt; i += 64) {
                const unsigned long long cm = fam[i], m = (unsigned long long)(base + i);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned long long key = ((unsigned long long)__popcll(code[k] ^ cm) << 40) | (m << 2) | (unsigned long long)k;
                    best = key < best ? key : best;
                }
            }
    }
    if (!have) return;
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off, 64);
        best = o < best ? o : best;
    }
    int id = -1, rot = -1, ham = -1;
    if (matching && (int)(best >> 40) <= a.max_hamming) {
        reason = CCAL_TAG_OK;
        ham = (int)(best >> 40); id = (int)((best >> 2) & 0x7fffffffull); rot = (int)(best & 3ull);
    }
    if (lane == 0) {
        a.reason[g] = reason; a.id[g] = id; a.rot[g] = rot; a.hamming[g] = ham;
        a.code[g] = (reason == CCAL_TAG_OUTSIDE || reason == CCAL_TAG_LOW_CONTRAST) ? 0ull : code[0];
        a.margin[g] = margin;
    }
    // 9. corners_out[i] = q[(i + 3 rot) mod 4]
    if (lane < 4) {
        const int src = (lane + 3 * (rot < 0 ? 0 : rot)) & 3;
        const double nan = __builtin_nan("");
        const double cx = src == 0 ? qx[0] : (src == 1 ? qx[1] : (src == 2 ? qx[2] : qx[3]));
        const double cy = src == 0 ? qy[0] : (src == 1 ? qy[1] : (src == 2 ? qy[2] : qy[3]));
        a.corners[8 * g + 2 * lane] = reason == CCAL_TAG_OK ? cx : nan;
        a.corners[8 * g + 2 * lane + 1] = reason == CCAL_TAG_OK ? cy : nan;
    }
}

// the ranges, and the table on its own: the entry points check the ranges before the image arguments, the table after
const char* tags_bad_params(int d, int border, int n_codes, int samples, double min_contrast, int max_border_errors, int max_hamming) {
    if (d < 3 || d > 8) return "d outside 3 .. 8";
    if (border < 1 || border > 2) return "border outside 1 .. 2";
    if (n_codes < 1) return "n_codes < 1";
    if (samples < 1 || samples > 4) return "samples outside 1 .. 4";
    if (!(min_contrast >= 0.0) || !std::isfinite(min_contrast)) return "min_contrast negative or not finite";
    if (max_border_errors < 0) return "max_border_errors < 0";
    if (max_hamming < 0 || max_hamming > d * d) return "max_hamming outside 0 .. d * d";
    return nullptr;
}

const char* tags_bad_codes(int d, const uint64_t* codes, int n_codes) {       // d and n_codes in range; codes == nullptr: nothing to test
    if (codes && d * d < 64)                              // at d = 8 every uint64 is a code: nothing to test, and no shift by 64
        for (int i = 0; i < n_codes; ++i)
            if (codes[i] >> (d * d)) return "a code of more than d * d bits";
    return nullptr;
}

hipError_t tags_enqueue(hipStream_t s, int dtype, const TagArgs& a) {
    static_assert(kTagMaxSide * kTagMaxSide <= 64 * kTagCellChunks, "three cells per lane hold the largest grid");
    const dim3 grid((unsigned)(((size_t)a.n + kTagWaves - 1) / kTagWaves));
    for_pix_type(dtype, [&](auto t) { hipLaunchKernelGGL(k_decode_tags<decltype(t)>, grid, dim3(64 * kTagWaves), 0, s, a); });
    return hipGetLastError();
}

namespace {

int tags_call(ccal_ctx* ctx, const char* where, const GreyBatch& b, const int64_t* offsets, const double* quads, int d, int border,
              const uint64_t* codes, int n_codes, int samples, double min_contrast, int max_border_errors, int max_hamming,
              int32_t* reason_out, int32_t* id_out, int32_t* rot_out, int32_t* hamming_out, double* corners_out, uint64_t* code_out, double* margin_out) {
    const BadArg bad{ ctx, where };
    if (const char* what = tags_bad_params(d, border, n_codes, samples, min_contrast, max_border_errors, max_hamming)) return bad(what);
    if (const char* what = b.bad()) return bad(what);
    if (const char* what = tags_bad_codes(d, codes, n_codes)) return bad(what);
    const int n_img = b.n_img;
    if (n_img == 0) return CCAL_OK;
    if (!b.images || !offsets || !codes || !reason_out || !id_out || !rot_out || !hamming_out) return bad("NULL argument");
    if (check_offsets(ctx, where, "offsets", offsets, (size_t)n_img, 0)) return CCAL_ERR_INVALID_ARG;
    if (offsets[n_img] > (int64_t)INT32_MAX) return bad("more than 2^31 - 1 quads");
    if (offsets[n_img] == 0) return CCAL_OK;
    if (!quads) return bad("NULL argument");
    // chunks of whole images: as many as keep the chunk's images (host call), quads and outputs within the limit, at least one
    const ImageChunks plan = image_chunks(offsets, (size_t)n_img, b.staged_bytes(1) + kTagPerImageBytes, kTagPerQuadBytes,
                                          test_chunk_bytes("CCAL_TEST_TAGS_CHUNK_BYTES", kTagChunkBytes));
    const std::vector<size_t>& cut = plan.cut;
    const size_t max_img = plan.max_img, max_quads = plan.max_rows;

    // one block for the largest chunk: family | offsets | images (host call) | quads | corners, margin | code | reason, id, rot, hamming
    CallBlock blk(ctx);
    const auto s_codes = blk.add<unsigned long long>((size_t)n_codes);
    const auto s_off = blk.add<int64_t>(max_img + 1);
    const auto s_img = blk.add<char>(b.staged_bytes(max_img));
    const auto s_quads = blk.add<double>(8 * max_quads);
    const auto s_corners = blk.add<double>(8 * max_quads);
    const auto s_margin = blk.add<double>(max_quads);
    const auto s_code = blk.add<unsigned long long>(max_quads);
    const auto s_reason = blk.add<int32_t>(max_quads);
    const auto s_id = blk.add<int32_t>(max_quads);
    const auto s_rot = blk.add<int32_t>(max_quads);
    const auto s_ham = blk.add<int32_t>(max_quads);
    if (!blk.alloc()) return blk.finish(where);

    TagArgs a = {};
    a.off = blk.at(s_off); a.quads = blk.at(s_quads); a.codes = blk.at(s_codes);
    a.reason = blk.at(s_reason); a.id = blk.at(s_id); a.rot = blk.at(s_rot); a.hamming = blk.at(s_ham);
    a.corners = blk.at(s_corners); a.code = blk.at(s_code); a.margin = blk.at(s_margin);
    a.W = b.width; a.H = b.height; a.d = d; a.border = border; a.n_codes = n_codes; a.S = samples;
    a.max_border = max_border_errors; a.max_hamming = max_hamming; a.min_contrast = min_contrast;
    blk.upload(s_codes, codes, (size_t)n_codes);

    for (size_t c = 0; c + 1 < cut.size() && blk.ok(); ++c) {
        const size_t k0 = cut[c], m = cut[c + 1] - k0;
        const size_t at = (size_t)offsets[k0], nq = (size_t)(offsets[k0 + m] - offsets[k0]);
        if (!nq) continue;
        a.n_img = (int32_t)m; a.q0 = offsets[k0]; a.n = (int64_t)nq;
        blk.poison(s_corners, s_margin);                 // the test hook's NaN over the doubles the kernel writes and never reads
        blk.upload(s_off, offsets + k0, m + 1);
        a.img = b.chunk(blk, s_img, k0, m);
        blk.upload(s_quads, quads + 8 * at, 8 * nq);
        if (blk.ok()) blk.note(tags_enqueue(ctx->stream, b.dtype, a));
        blk.download(reason_out + at, a.reason, nq);
        blk.download(id_out + at, a.id, nq);
        blk.download(rot_out + at, a.rot, nq);
        blk.download(hamming_out + at, a.hamming, nq);
        blk.download(corners_out ? corners_out + 8 * at : nullptr, a.corners, 8 * nq);
        blk.download(code_out ? code_out + at : nullptr, a.code, nq);
        blk.download(margin_out ? margin_out + at : nullptr, a.margin, nq);
    }                                                    // the next chunk's uploads follow these copies on the same stream
    return blk.finish(where);
}

}  // namespace
}  // namespace ccal

using namespace ccal;

extern "C" {

int ccal_decode_tags_batch(ccal_ctx* ctx, int dtype, int width, int height, int n_img, const void* images, const int64_t* offsets,
                           const double* quads, int d, int border, const uint64_t* codes, int n_codes, int samples, double min_contrast,
                           int max_border_errors, int max_hamming, int32_t* reason_out, int32_t* id_out, int32_t* rot_out,
                           int32_t* hamming_out, double* corners_out, uint64_t* code_out, double* margin_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    return tags_call(ctx, "ccal_decode_tags_batch", GreyBatch{ dtype, width, height, n_img, images, false }, offsets, quads, d, border, codes,
                     n_codes, samples, min_contrast, max_border_errors, max_hamming, reason_out, id_out, rot_out, hamming_out, corners_out,
                     code_out, margin_out);
    CCAL_API_CATCH(ctx)
}

int ccal_decode_tags_dev(ccal_ctx* ctx, int dtype, int width, int height, int n_img, const void* images_dev, const int64_t* offsets,
                         const double* quads, int d, int border, const uint64_t* codes, int n_codes, int samples, double min_contrast,
                         int max_border_errors, int max_hamming, int32_t* reason_out, int32_t* id_out, int32_t* rot_out,
                         int32_t* hamming_out, double* corners_out, uint64_t* code_out, double* margin_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    return tags_call(ctx, "ccal_decode_tags_dev", GreyBatch{ dtype, width, height, n_img, images_dev, true }, offsets, quads, d, border, codes,
                     n_codes, samples, min_contrast, max_border_errors, max_hamming, reason_out, id_out, rot_out, hamming_out, corners_out,
                     code_out, margin_out);
    CCAL_API_CATCH(ctx)
}

}  // extern "C"

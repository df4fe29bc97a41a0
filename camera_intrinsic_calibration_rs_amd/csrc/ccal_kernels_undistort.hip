// Applying a calibration: GenericModel::project / unproject over arrays of points, estimate_new_camera_matrix_for_undistort,
// init_undistort_map and remap (the tail of examples/convert_model.rs:27-29 and examples/test_pnp.rs:51,78-80).
//   k_project_points<MODEL>    xyz [n][3] -> uv [n][2], valid [n]            f64, grid-stride
//   k_unproject_points<MODEL>  uv [n][2]  -> ray [n][3], valid [n]           f64, grid-stride
//   k_undistort_map<MODEL>     K, R -> xmap, ymap [new_h][new_w] f32         f64 arithmetic, one output pixel per lane
//   k_remap<T, C>              bilinear resampling of n_img interleaved images through ONE map; four neighbouring output
//                              pixels per lane (one, two or three dwords of output), the loop over the images inside
// Remap semantics (fixed by this project, the `image` crate is not part of the reference tree): a map entry (mx, my) is valid
// iff 0 <= mx <= W-1 and 0 <= my <= H-1 (NaN and +-inf fail, -0.0 counts as 0); an invalid entry writes 0 in every channel;
// a valid one, in f32: x0 = floor(mx), ax = mx - x0, x1 = min(x0 + 1, W-1), the same for y,
// val = (1-ay) ((1-ax) p00 + ax p01) + ay ((1-ax) p10 + ax p11), output = (T)floorf(val + 0.5f) clamped to Pix<T>::hi (ccal_pix.hpp).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>

#include "ccal_call.hpp"
#include "ccal_device.hpp"
#include "ccal_model_inverse.hpp"
#include "ccal_pix.hpp"

struct ccal_undistort_map {
    ccal_ctx* ctx = nullptr;
    float* d_maps = nullptr;           // ONE block of the context's allocator: xmap [h][w], then ymap [h][w] at the next 256-byte boundary
    int32_t w = 0, h = 0;
    size_t stride() const { return ((size_t)w * h + 63) & ~(size_t)63; }      // floats from xmap to ymap: both take 16-byte loads
    float* xmap() const { return d_maps; }
    float* ymap() const { return d_maps + stride(); }
};

namespace ccal {

// The model parameters travel in the argument block, in the kernels' canonical order (OPENCV5: k1, k2, p1, p2, k3 - permuted at
// the API boundary from ccal_model_conventions.ocv5_order, like ccal_convert_model does), with the context's two thresholds.
struct PointArgs {
    double th[CCAL_PMAX];
    ModelRt rt;
    int64_t n;
    const double* in;                  // xyz [n][3] (project) or uv [n][2] (unproject)
    double* out;                       // uv [n][2] or ray [n][3]
    uint8_t* valid;                    // [n]
};
struct MapArgs {
    double th[CCAL_PMAX];
    ModelRt rt;
    double fx, fy, cx, cy;             // the new camera matrix
    double R[9];                       // row-major; the ray of an output pixel is R^T ((x - cx) / fx, (y - cy) / fy, 1)
    int32_t w, h;
    float* xmap; float* ymap;
};

template <int MODEL>
__device__ __forceinline__ void theta_from_args(const double* a_th, const ModelRt& rt, double* th) {
#pragma unroll
    for (int i = 0; i < model_np(MODEL); ++i) th[i] = a_th[i];
    th[model_np(MODEL)] = rt.kb4_eps;
}

template <int MODEL>
__global__ __launch_bounds__(256) void k_project_points(const PointArgs a) {
    double th[th_len<MODEL>()];
    theta_from_args<MODEL>(a.th, a.rt, th);
    const double nan = __builtin_nan("");
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
        const double x = a.in[3 * i], y = a.in[3 * i + 1], z = a.in[3 * i + 2];
        double u = nan, v = nan;
        const bool ok = project_valid<MODEL>(th, x, y, z);
        if (ok) project_uv<MODEL>(th, x, y, z, u, v);
        *reinterpret_cast<double2*>(a.out + 2 * i) = make_double2(u, v);
        a.valid[i] = ok ? 1 : 0;
    }
}

template <int MODEL>
__global__ __launch_bounds__(256) void k_unproject_points(const PointArgs a) {
    double th[th_len<MODEL>()];
    theta_from_args<MODEL>(a.th, a.rt, th);
    const double nan = __builtin_nan("");
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
        const double2 p = *reinterpret_cast<const double2*>(a.in + 2 * i);
        double x = nan, y = nan, z = nan;
        const bool ok = unproject_ray<MODEL>(th, a.rt.unproject_eps, p.x, p.y, x, y, z);
        if (!ok) { x = nan; y = nan; z = nan; }
        a.out[3 * i] = x; a.out[3 * i + 1] = y; a.out[3 * i + 2] = z;
        a.valid[i] = ok ? 1 : 0;
    }
}

// One output pixel per lane, rows contiguous across lanes: each of the two stores of a wavefront is 256 contiguous bytes.
template <int MODEL>
__global__ __launch_bounds__(256) void k_undistort_map(const MapArgs a) {
    double th[th_len<MODEL>()];
    theta_from_args<MODEL>(a.th, a.rt, th);
    const uint32_t n = (uint32_t)a.w * (uint32_t)a.h;          // <= INT32_MAX (checked at the API)
    const double ifx = 1.0 / a.fx, ify = 1.0 / a.fy;
    const float nanf = __builtin_nanf("");
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const uint32_t py = i / (uint32_t)a.w, px = i - py * (uint32_t)a.w;
        const double xn = ((double)px - a.cx) * ifx, yn = ((double)py - a.cy) * ify;
        const double x = a.R[0] * xn + a.R[3] * yn + a.R[6];
        const double y = a.R[1] * xn + a.R[4] * yn + a.R[7];
        const double z = a.R[2] * xn + a.R[5] * yn + a.R[8];
        float mu = nanf, mv = nanf;
        if (project_valid<MODEL>(th, x, y, z)) {
            double u, v;
            project_uv<MODEL>(th, x, y, z, u, v);
            mu = (float)u; mv = (float)v;
        }
        a.xmap[i] = mu; a.ymap[i] = mv;
    }
}

struct RemapArgs {
    const float* xmap; const float* ymap;       // [n_pix]
    int64_t n_pix;                              // output pixels per image (map width x height)
    int32_t src_w, src_h;
    int32_t n_img, img_per_y;                   // images of the batch; images one blockIdx.y works through
    const void* src; void* dst;
};

// One tap set of an output pixel: element offsets of the four neighbours inside an image, the two weights, validity.
struct Tap { int32_t o00, o01, o10, o11; float ax, ay; bool ok; };

template <int C>
__device__ __forceinline__ Tap make_tap(float mx, float my, int32_t W, int32_t H) {
    Tap t;
    t.ok = mx >= 0.0f && mx <= (float)(W - 1) && my >= 0.0f && my <= (float)(H - 1);      // false for NaN and +-inf
    if (!t.ok) { mx = 0.0f; my = 0.0f; }
    const float fx0 = floorf(mx), fy0 = floorf(my);
    const int32_t x0 = (int32_t)fx0, y0 = (int32_t)fy0;
    const int32_t x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    t.ax = mx - fx0; t.ay = my - fy0;
    t.o00 = (y0 * W + x0) * C; t.o01 = (y0 * W + x1) * C; t.o10 = (y1 * W + x0) * C; t.o11 = (y1 * W + x1) * C;
    return t;
}

template <class T>
__device__ __forceinline__ uint32_t blend(const Tap& t, T p00, T p01, T p10, T p11) {
    const float top = (1.0f - t.ax) * (float)p00 + t.ax * (float)p01;
    const float bot = (1.0f - t.ax) * (float)p10 + t.ax * (float)p11;
    const float val = (1.0f - t.ay) * top + t.ay * bot;
    const float r = fminf(fmaxf(floorf(val + 0.5f), 0.0f), (float)Pix<T>::hi);
    return t.ok ? (uint32_t)r : 0u;
}

// Four neighbouring output pixels (flat index 4 g .. 4 g + 3 of the map) per lane: 4 C sizeof(T) = 4, 8 or 12 bytes of output,
// stored as whole dwords when the image's first byte is dword-aligned; the map is read once (two 16-byte loads) and kept in
// registers for every image of this blockIdx.y's share of the batch.  All gathers of an image (16 C loads) are independent.
template <class T, int C>
__global__ __launch_bounds__(256) void k_remap(const RemapArgs a) {
    constexpr int PX = 4, NB = PX * C * (int)sizeof(T), ND = NB / 4;
    const int64_t n_groups = (a.n_pix + PX - 1) / PX;
    const int64_t img_in = (int64_t)a.src_w * a.src_h * C, img_out = a.n_pix * C;      // elements per image
    const int32_t img0 = blockIdx.y * a.img_per_y, img1 = min(img0 + a.img_per_y, a.n_img);
    const T* src = static_cast<const T*>(a.src);
    T* dst = static_cast<T*>(a.dst);
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n_groups; g += (int64_t)gridDim.x * 256) {
        const int64_t p0 = g * PX;
        const bool full = p0 + PX <= a.n_pix;
        float mx[PX], my[PX];
        if (full) {
            const float4 vx = *reinterpret_cast<const float4*>(a.xmap + p0), vy = *reinterpret_cast<const float4*>(a.ymap + p0);
            mx[0] = vx.x; mx[1] = vx.y; mx[2] = vx.z; mx[3] = vx.w;
            my[0] = vy.x; my[1] = vy.y; my[2] = vy.z; my[3] = vy.w;
        } else {
#pragma unroll
            for (int k = 0; k < PX; ++k) {
                const bool in = p0 + k < a.n_pix;
                mx[k] = in ? a.xmap[in ? p0 + k : 0] : -1.0f;
                my[k] = in ? a.ymap[in ? p0 + k : 0] : -1.0f;
            }
        }
        Tap t[PX];
#pragma unroll
        for (int k = 0; k < PX; ++k) t[k] = make_tap<C>(mx[k], my[k], a.src_w, a.src_h);
#pragma unroll 2
        for (int32_t im = img0; im < img1; ++im) {
            const T* s = src + (int64_t)im * img_in;
            T* d = dst + (int64_t)im * img_out + p0 * C;
            uint32_t o[PX * C];
#pragma unroll
            for (int k = 0; k < PX; ++k) {
#pragma unroll
                for (int c = 0; c < C; ++c)
                    o[k * C + c] = blend<T>(t[k], s[t[k].o00 + c], s[t[k].o01 + c], s[t[k].o10 + c], s[t[k].o11 + c]);
            }
            if (full && (reinterpret_cast<uintptr_t>(d) & 3u) == 0) {
                uint32_t w[ND];
#pragma unroll
                for (int j = 0; j < ND; ++j) {
                    if constexpr (sizeof(T) == 1) w[j] = o[4 * j] | (o[4 * j + 1] << 8) | (o[4 * j + 2] << 16) | (o[4 * j + 3] << 24);
                    else w[j] = o[2 * j] | (o[2 * j + 1] << 16);
                }
                uint32_t* dw = reinterpret_cast<uint32_t*>(d);
                if constexpr (ND == 1) dw[0] = w[0];
                else if constexpr (ND == 2) *reinterpret_cast<uint2*>(dw) = make_uint2(w[0], w[1]);
                else { dw[0] = w[0]; dw[1] = w[1]; dw[2] = w[2]; }
            } else {
#pragma unroll
                for (int k = 0; k < PX; ++k) {
                    if (p0 + k < a.n_pix) {
#pragma unroll
                        for (int c = 0; c < C; ++c) d[k * C + c] = (T)o[k * C + c];
                    }
                }
            }
        }
    }
}

namespace {

inline int grid_for(int64_t n) { return (int)std::min<int64_t>(std::max<int64_t>((n + 255) / 256, 1), 2048); }

template <int M> struct LaunchProject { static void go(int g, hipStream_t st, const PointArgs& a) { hipLaunchKernelGGL(k_project_points<M>, dim3(g), dim3(256), 0, st, a); } };
template <int M> struct LaunchUnproject { static void go(int g, hipStream_t st, const PointArgs& a) { hipLaunchKernelGGL(k_unproject_points<M>, dim3(g), dim3(256), 0, st, a); } };
template <int M> struct LaunchMap { static void go(int g, hipStream_t st, const MapArgs& a) { hipLaunchKernelGGL(k_undistort_map<M>, dim3(g), dim3(256), 0, st, a); } };

// project (in_w = 3, out_w = 2) or unproject (2, 3) of n host points through one device block [in | out | valid]
int points_call(ccal_ctx* ctx, bool project, int model, const double* params, int64_t n, const double* in, double* out, uint8_t* valid_out,
                const char* where) {
    if (!params || n < 0 || (n > 0 && (!in || !out || !valid_out))) { ctx->err = std::string(where) + ": invalid argument"; return CCAL_ERR_INVALID_ARG; }
    const int rc = check_model(ctx, model, where);
    if (rc != CCAL_OK) return rc;
    if (n == 0) return CCAL_OK;
    const size_t in_w = project ? 3 : 2, out_w = project ? 2 : 3;
    CallBlock blk(ctx);
    const auto s_in = blk.add<double>(in_w * (size_t)n);
    const auto s_out = blk.add<double>(out_w * (size_t)n);
    const auto s_valid = blk.add<uint8_t>((size_t)n);
    if (!blk.alloc()) return blk.finish(where);
    blk.poison(s_in, s_valid);
    PointArgs a;
    canonical_theta(ctx, model, params, a.th, &a.rt);
    a.n = n; a.in = blk.at(s_in); a.out = blk.at(s_out); a.valid = blk.at(s_valid);
    blk.upload(s_in, in, in_w * (size_t)n);
    if (blk.ok()) {
        if (project) launch_model<LaunchProject>(model, grid_for(n), ctx->stream, a);
        else launch_model<LaunchUnproject>(model, grid_for(n), ctx->stream, a);
        blk.launched();
    }
    blk.download(out, a.out, out_w * (size_t)n);
    blk.download(valid_out, a.valid, (size_t)n);
    return blk.finish(where);
}

int map_alloc(ccal_ctx* ctx, int32_t w, int32_t h, ccal_undistort_map** out) {
    if ((int64_t)w * h > (int64_t)INT32_MAX) { ctx->err = "ccal_undistort_map: map too large"; return CCAL_ERR_INVALID_ARG; }
    std::unique_ptr<ccal_undistort_map> m(new ccal_undistort_map());
    m->w = w; m->h = h;
    const size_t bytes = 2 * sizeof(float) * m->stride();
    HIP_TRY(ctx, ctx_dev_alloc(ctx, (void**)&m->d_maps, bytes));
    m->ctx = ctx;
    ++ctx->n_problems;                 // a map holds its context like a problem does (deferred ccal_ctx_destroy)
    *out = m.release();
    const hipError_t e = test_poison_f64(ctx, (*out)->d_maps, bytes, false, ctx->stream);
    if (e != hipSuccess) { ctx->err = std::string("ccal_undistort_map: ") + hipGetErrorString(e); ccal_undistort_map_destroy(*out); *out = nullptr; return CCAL_ERR_HIP; }
    return CCAL_OK;
}

bool pix_combo_ok(int dtype, int channels) {
    return (dtype == CCAL_PIX_U8 && (channels == 1 || channels == 3)) || (dtype == CCAL_PIX_U16 && channels == 1);
}

void remap_launch(const ccal_undistort_map* map, int dtype, int channels, int src_w, int src_h, int n_img, const void* d_src, void* d_dst,
                  hipStream_t st) {
    RemapArgs a;
    a.xmap = map->xmap(); a.ymap = map->ymap(); a.n_pix = (int64_t)map->w * map->h;
    a.src_w = src_w; a.src_h = src_h; a.n_img = n_img; a.src = d_src; a.dst = d_dst;
    const int64_t n_groups = (a.n_pix + 3) / 4;
    const int gx = grid_for(n_groups);
    // the batch is cut over blockIdx.y only as far as it takes to fill the GPU (about 2048 workgroups): every lane keeps its
    // four map entries for all the images of its share
    const int want_y = std::max(1, 2048 / gx);
    const int gy = std::min({ n_img, want_y, 65535 });
    a.img_per_y = (n_img + gy - 1) / gy;
    const dim3 grid(gx, (n_img + a.img_per_y - 1) / a.img_per_y);
    if (dtype == CCAL_PIX_U16) hipLaunchKernelGGL((k_remap<uint16_t, 1>), grid, dim3(256), 0, st, a);
    else if (channels == 3) hipLaunchKernelGGL((k_remap<uint8_t, 3>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_remap<uint8_t, 1>), grid, dim3(256), 0, st, a);
}

int remap_check(const ccal_undistort_map* map, int dtype, int channels, int src_w, int src_h, int n_img, const void* src, void* dst) {
    ccal_ctx* ctx = map->ctx;
    if (!pix_combo_ok(dtype, channels) || src_w <= 0 || src_h <= 0 || n_img <= 0 || !src || !dst) { ctx->err = "ccal_remap: invalid argument"; return CCAL_ERR_INVALID_ARG; }
    // the kernel addresses the neighbours of a pixel by 32-bit element offsets inside one image and compares map entries with
    // (float)(W - 1), (float)(H - 1), which must be exact
    if (src_w > (1 << 24) || src_h > (1 << 24) || (int64_t)src_w * src_h * channels > (int64_t)INT32_MAX) { ctx->err = "ccal_remap: source image too large"; return CCAL_ERR_INVALID_ARG; }
    return CCAL_OK;
}

}  // namespace
}  // namespace ccal

using namespace ccal;

extern "C" {

int ccal_project_points(ccal_ctx* ctx, int model, const double* params, int64_t n, const double* xyz, double* uv_out, uint8_t* valid_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    return points_call(ctx, true, model, params, n, xyz, uv_out, valid_out, "ccal_project_points");
    CCAL_API_CATCH(ctx)
}

int ccal_unproject_points(ccal_ctx* ctx, int model, const double* params, int64_t n, const double* uv, double* rays_out, uint8_t* valid_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    return points_call(ctx, false, model, params, n, uv, rays_out, valid_out, "ccal_unproject_points");
    CCAL_API_CATCH(ctx)
}

int ccal_estimate_new_camera_matrix(ccal_ctx* ctx, int model, const double* params, int width, int height, double balance,
                                    int new_w, int new_h, double* K_out) {
    if (!ctx) return CCAL_ERR_INVALID_ARG;
    CCAL_API_TRY
    if (!params || !K_out || width <= 0 || height <= 0 || new_w < 0 || new_h < 0 || (new_w == 0) != (new_h == 0) ||
        !(balance >= 0.0 && balance <= 1.0)) { ctx->err = "ccal_estimate_new_camera_matrix: invalid argument"; return CCAL_ERR_INVALID_ARG; }
    const int rc0 = check_model(ctx, model, "ccal_estimate_new_camera_matrix");
    if (rc0 != CCAL_OK) return rc0;
    if (new_w == 0) { new_w = width; new_h = height; }
    const double cx = params[2], cy = params[3];
    const double uv[8] = { cx, 0.0, (double)(width - 1), cy, cx, (double)(height - 1), 0.0, cy };
    double rays[12];
    uint8_t ok[4];
    const int rc = points_call(ctx, false, model, params, 4, uv, rays, ok, "ccal_estimate_new_camera_matrix");
    if (rc != CCAL_OK) return rc;
    double min_x = INFINITY, max_x = -INFINITY, min_y = INFINITY, max_y = -INFINITY;
    for (int i = 0; i < 4; ++i) {
        if (!ok[i] || !(rays[3 * i + 2] > 0.0)) { ctx->err = "ccal_estimate_new_camera_matrix: an edge midpoint has no ray in front of the camera"; return CCAL_NO_RESULT; }
        const double x = rays[3 * i] / rays[3 * i + 2], y = rays[3 * i + 1] / rays[3 * i + 2];
        min_x = std::min(min_x, x); max_x = std::max(max_x, x); min_y = std::min(min_y, y); max_y = std::max(max_y, y);
    }
    min_x = std::fabs(min_x); min_y = std::fabs(min_y);
    const double rx = (double)new_w / (min_x + max_x), ry = (double)new_h / (min_y + max_y);
    const double f_a = std::max(rx, ry), f_b = std::min(rx, ry);
    const double f = balance * f_a + (1.0 - balance) * f_b;
    const double K[9] = { f, 0.0, (double)new_w * min_x / (min_x + max_x), 0.0, f, (double)new_h * min_y / (min_y + max_y), 0.0, 0.0, 1.0 };
    for (int i = 0; i < 9; ++i) if (!std::isfinite(K[i])) { ctx->err = "ccal_estimate_new_camera_matrix: degenerate field of view"; return CCAL_NO_RESULT; }
    std::memcpy(K_out, K, sizeof(K));
    return CCAL_OK;
    CCAL_API_CATCH(ctx)
}

int ccal_undistort_map_create(ccal_ctx* ctx, int model, const double* params, const double* K, const double* R, int new_w, int new_h,
                              ccal_undistort_map** out) {
    if (!ctx || !out) return CCAL_ERR_INVALID_ARG;
    *out = nullptr;
    CCAL_API_TRY
    if (!params || !K || new_w <= 0 || new_h <= 0 || !(K[0] != 0.0) || !(K[4] != 0.0) || !std::isfinite(K[0]) || !std::isfinite(K[4]) ||
        !std::isfinite(K[2]) || !std::isfinite(K[5])) { ctx->err = "ccal_undistort_map_create: invalid argument"; return CCAL_ERR_INVALID_ARG; }
    const int rc0 = check_model(ctx, model, "ccal_undistort_map_create");
    if (rc0 != CCAL_OK) return rc0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ccal_undistort_map* m = nullptr;
    const int rc = map_alloc(ctx, new_w, new_h, &m);
    if (rc != CCAL_OK) return rc;
    MapArgs a;
    canonical_theta(ctx, model, params, a.th, &a.rt);
    a.fx = K[0]; a.fy = K[4]; a.cx = K[2]; a.cy = K[5];
    static const double eye[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };
    std::memcpy(a.R, R ? R : eye, sizeof(a.R));
    a.w = new_w; a.h = new_h; a.xmap = m->xmap(); a.ymap = m->ymap();
    launch_model<LaunchMap>(model, grid_for((int64_t)new_w * new_h), ctx->stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { ctx->err = std::string("k_undistort_map: ") + hipGetErrorString(e); ccal_undistort_map_destroy(m); return CCAL_ERR_HIP; }
    *out = m;
    return CCAL_OK;
    CCAL_API_CATCH(ctx)
}

int ccal_undistort_map_from_host(ccal_ctx* ctx, const float* xmap, const float* ymap, int w, int h, ccal_undistort_map** out) {
    if (!ctx || !out) return CCAL_ERR_INVALID_ARG;
    *out = nullptr;
    CCAL_API_TRY
    if (!xmap || !ymap || w <= 0 || h <= 0) { ctx->err = "ccal_undistort_map_from_host: invalid argument"; return CCAL_ERR_INVALID_ARG; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ccal_undistort_map* m = nullptr;
    const int rc = map_alloc(ctx, w, h, &m);
    if (rc != CCAL_OK) return rc;
    const size_t bytes = sizeof(float) * (size_t)w * (size_t)h;
    hipError_t e = hipMemcpyAsync(m->xmap(), xmap, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(m->ymap(), ymap, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);          // the caller's arrays are free again on return
    if (e != hipSuccess) { ctx->err = std::string("ccal_undistort_map_from_host: ") + hipGetErrorString(e); ccal_undistort_map_destroy(m); return CCAL_ERR_HIP; }
    *out = m;
    return CCAL_OK;
    CCAL_API_CATCH(ctx)
}

int ccal_undistort_map_download(ccal_undistort_map* map, float* xmap_out, float* ymap_out) {
    if (!map || !map->ctx) return CCAL_ERR_INVALID_ARG;
    ccal_ctx* ctx = map->ctx;
    CCAL_API_TRY
    if (!xmap_out || !ymap_out) { ctx->err = "ccal_undistort_map_download: invalid argument"; return CCAL_ERR_INVALID_ARG; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t bytes = sizeof(float) * (size_t)map->w * (size_t)map->h;
    HIP_TRY(ctx, hipMemcpyAsync(xmap_out, map->xmap(), bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ymap_out, map->ymap(), bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CCAL_OK;
    CCAL_API_CATCH(ctx)
}

void ccal_undistort_map_destroy(ccal_undistort_map* map) {
    if (!map) return;
    ccal_ctx* ctx = map->ctx;
    if (ctx && map->d_maps) {
        // nothing may still read the maps when the block goes back to the context (a caller-provided stream may be gone already
        // when a binding's garbage collector gets here: the device is drained then)
        (void)hipSetDevice(ctx->device);
        if (ctx->own_stream && ctx->stream) (void)hipStreamSynchronize(ctx->stream); else (void)hipDeviceSynchronize();
        (void)hipGetLastError();
        ctx_release(ctx, map->d_maps, false);
    }
    delete map;
    if (ctx) ctx_unref(ctx);
}

int ccal_remap(ccal_undistort_map* map, int dtype, int channels, int src_w, int src_h, int n_img, const void* src, void* dst) {
    if (!map || !map->ctx) return CCAL_ERR_INVALID_ARG;
    ccal_ctx* ctx = map->ctx;
    CCAL_API_TRY
    const int rc0 = remap_check(map, dtype, channels, src_w, src_h, n_img, src, dst);
    if (rc0 != CCAL_OK) return rc0;
    const size_t es = dtype == CCAL_PIX_U16 ? 2 : 1;
    const size_t b_src = es * (size_t)channels * (size_t)src_w * (size_t)src_h * (size_t)n_img;
    const size_t b_dst = es * (size_t)channels * (size_t)map->w * (size_t)map->h * (size_t)n_img;
    CallBlock blk(ctx);
    const auto s_src = blk.add<char>(b_src);
    const auto s_dst = blk.add<char>(b_dst);
    if (!blk.alloc()) return blk.finish("ccal_remap");
    blk.poison(s_src, s_dst);
    blk.upload(s_src, src, b_src);
    if (blk.ok()) {
        remap_launch(map, dtype, channels, src_w, src_h, n_img, blk.at(s_src), blk.at(s_dst), ctx->stream);
        blk.launched();
    }
    blk.download(dst, blk.at(s_dst), b_dst);
    return blk.finish("ccal_remap");
    CCAL_API_CATCH(ctx)
}

int ccal_remap_dev(ccal_undistort_map* map, int dtype, int channels, int src_w, int src_h, int n_img, const void* src_dev, void* dst_dev) {
    if (!map || !map->ctx) return CCAL_ERR_INVALID_ARG;
    ccal_ctx* ctx = map->ctx;
    CCAL_API_TRY
    const int rc0 = remap_check(map, dtype, channels, src_w, src_h, n_img, src_dev, dst_dev);
    if (rc0 != CCAL_OK) return rc0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    remap_launch(map, dtype, channels, src_w, src_h, n_img, src_dev, dst_dev, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    return CCAL_OK;
    CCAL_API_CATCH(ctx)
}

}  // extern "C"

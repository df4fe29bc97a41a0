// What the two pose-initialisation kernels share (k_pose_init, ccal_kernels_init.hip: planar targets; k_pose_pnp,
// ccal_kernels_pnp.hip: any other): the unprojection to normalised image points and the argument block.
#pragma once
#include "ccal_device.hpp"
#include "ccal_internal.hpp"

namespace ccal {

// Not a camera model of the engine: the one-parameter division model of the two-frame initialisation (init_pose,
// src/optimization/linear.rs:5-21) as an unprojection variant of k_pose_init.  th = [half, half, w/2, h/2, lambda]:
// bearing = ((p2d - c) / half) / (1 + lambda r^2).
constexpr int kUnprojDivision = 100;

// unproject + divide by z: the model inverse as published (UCM/EUCM closed form, Usenko et al. 2018;
// KB4 Newton on theta; OPENCV5 fixed-point undistortion).  Returns false where the reference's
// `unproject` yields None (outside the model's domain) or the ray is not in front of the camera.
template <int MODEL>
__device__ __forceinline__ bool unproject_normalized(const double* th, double small_radius, double u, double v, double& xn, double& yn) {
    const double mx = (u - th[2]) / th[0], my = (v - th[3]) / th[1];
    const double r2 = mx * mx + my * my;
    if constexpr (MODEL == kUnprojDivision) {
        const double sc = 1.0 + th[4] * r2;
        if (!(sc > 1e-9)) return false;                         // beyond the division model's domain: no ray
        xn = mx / sc; yn = my / sc;
        return true;
    } else if constexpr (MODEL == kUCM || MODEL == kEUCM) {
        const double alpha = th[4], beta = (MODEL == kEUCM) ? th[5] : 1.0;
        if (alpha > 0.5 && r2 > 1.0 / (beta * (2.0 * alpha - 1.0))) return false;
        const double t1 = 1.0 - (2.0 * alpha - 1.0) * beta * r2;
        if (t1 < 0.0) return false;
        const double den = alpha * sqrt(t1) + (1.0 - alpha);
        const double k = (1.0 - alpha * alpha * beta * r2) / den;
        if (!(den > 0.0) || !(k > 1e-3) || !(k < __builtin_inf())) return false;      // alpha = 1 on the domain's edge: 0 / 0
        xn = mx / k; yn = my / k;
        return true;
    } else if constexpr (MODEL == kKB4) {
        const double r = sqrt(r2);
        if (r < small_radius) { xn = mx; yn = my; return true; }
        double t = r;
        for (int it = 0; it < 10; ++it) {
            const double t2 = t * t;
            const double f = t * (1.0 + t2 * (th[4] + t2 * (th[5] + t2 * (th[6] + t2 * th[7])))) - r;
            const double fp = 1.0 + t2 * (3.0 * th[4] + t2 * (5.0 * th[5] + t2 * (7.0 * th[6] + t2 * 9.0 * th[7])));
            t -= f / fp;
        }
        if (!(t > 0.0) || !(t < 1.5)) return false;             // theta < ~86 deg: in front of the camera
        const double tt = t * t;                                // accept only if re-projection reproduces the input (as OPENCV5 below)
        if (!(fabs(t * (1.0 + tt * (th[4] + tt * (th[5] + tt * (th[6] + tt * th[7])))) - r) < 1e-9)) return false;
        const double s = tan(t) / r;
        xn = mx * s; yn = my * s;
        return true;
    } else {
        const double k1 = th[OCV5_K1], k2 = th[OCV5_K2], p1 = th[OCV5_P1], p2 = th[OCV5_P2], k3 = th[OCV5_K3];
        double x = mx, y = my;
        for (int it = 0; it < 25; ++it) {
            const double q = x * x + y * y;
            const double rad = 1.0 + q * (k1 + q * (k2 + q * k3));
            const double dx = 2.0 * p1 * x * y + p2 * (q + 2.0 * x * x);
            const double dy = p1 * (q + 2.0 * y * y) + 2.0 * p2 * x * y;
            x = (mx - dx) / rad; y = (my - dy) / rad;
        }
        // accept only if re-projection reproduces the input
        const double q = x * x + y * y, rad = 1.0 + q * (k1 + q * (k2 + q * k3));
        const double ex = x * rad + 2.0 * p1 * x * y + p2 * (q + 2.0 * x * x) - mx;
        const double ey = y * rad + p1 * (q + 2.0 * y * y) + 2.0 * p2 * x * y - my;
        if (!(fabs(ex) + fabs(ey) < 1e-9)) return false;
        xn = x; yn = y;
        return true;
    }
}

struct InitArgs {
    const float* x; const float* y; const float* z; const float* u; const float* v;
    const int64_t* obs_off; const int32_t* list; int32_t n_list, cam;
    const double* intr;
    double* poses_obs;      // [n_obs][6]  T_cam_board
    int32_t* valid_obs;     // [n_obs]     number of corners used, 0 = no pose
    int32_t min_points;
    ModelRt rt;             // the context's run-time conventions
    double division[5];     // kUnprojDivision only: th as above
};

inline InitArgs pose_init_args(const ccal_problem* p, int cam) {
    InitArgs a = {};
    a.x = p->d_x; a.y = p->d_y; a.z = p->d_z; a.u = p->d_u; a.v = p->d_v;
    a.obs_off = p->d_obs_off; a.list = p->cams[cam].d_obs; a.n_list = (int32_t)p->cams[cam].obs.size(); a.cam = cam;
    return a;
}

// init_pose of the two-frame initialisation: centre and scale from the camera's image size, as linear.rs:6-9
inline void division_theta(const ccal_problem* p, int cam, double lambda, double* th) {
    const double hw = 0.5 * p->cams[cam].width, hh = 0.5 * p->cams[cam].height, half = hw > hh ? hw : hh;
    th[0] = half; th[1] = half; th[2] = hw; th[3] = hh; th[4] = lambda;
}

}  // namespace ccal

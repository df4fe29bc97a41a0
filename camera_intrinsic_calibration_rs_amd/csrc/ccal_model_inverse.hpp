// GenericModel::unproject and the validity test of GenericModel::project for the four models, shared by convert_model's ray
// kernel (ccal_convert.hip) and the point / undistortion-map kernels (ccal_kernels_undistort.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "ccal_device.hpp"

namespace ccal {

// Model inverse as published (UCM/EUCM: Usenko et al. 2018; KB4: Newton on theta; OPENCV5: fixed-point
// undistortion); rays may point backwards (z <= 0) for fisheye models.  false = `unproject` gives None.
// The contract (include/ccal.h, ccal_unproject_points): true means the ray re-projects onto the pixel - the iterative
// inverses accept their last iterate only if its residual in normalised units is below kUnprojectAccept, the closed form
// only if its denominator and norm are positive finite numbers (alpha = 1 on the domain's edge gives 0 / 0).
constexpr double kUnprojectAccept = 1e-9;
template <int MODEL>
__device__ bool unproject_ray(const double* th, double small_radius, double u, double v, double& x, double& y, double& z) {
    const double mx = (u - th[2]) / th[0], my = (v - th[3]) / th[1];
    const double r2 = mx * mx + my * my;
    if constexpr (MODEL == kUCM || MODEL == kEUCM) {
        const double alpha = th[4], beta = (MODEL == kEUCM) ? th[5] : 1.0;
        if (alpha > 0.5 && r2 > 1.0 / (beta * (2.0 * alpha - 1.0))) return false;
        const double t1 = 1.0 - (2.0 * alpha - 1.0) * beta * r2;
        if (t1 < 0.0) return false;
        const double den = alpha * sqrt(t1) + (1.0 - alpha);
        const double mz = (1.0 - beta * alpha * alpha * r2) / den;
        const double n = sqrt(r2 + mz * mz);
        if (!(den > 0.0) || !(n > 0.0) || !(n < __builtin_inf())) return false;
        x = mx / n; y = my / n; z = mz / n;
        return true;
    } else if constexpr (MODEL == kKB4) {
        const double r = sqrt(r2);
        if (r < small_radius) { x = mx; y = my; z = 1.0; return true; }
        double t = r;
        for (int it = 0; it < 20; ++it) {
            const double t2 = t * t;
            const double f = t * (1.0 + t2 * (th[4] + t2 * (th[5] + t2 * (th[6] + t2 * th[7])))) - r;
            const double fp = 1.0 + t2 * (3.0 * th[4] + t2 * (5.0 * th[5] + t2 * (7.0 * th[6] + t2 * 9.0 * th[7])));
            const double dt = f / fp;
            t -= dt;
            if (fabs(dt) < 1e-14) break;
        }
        if (!(t > 0.0) || !(t < 3.141592653589793)) return false;
        const double tt = t * t;            // the iteration is accepted wherever it stops only if theta_d(t) = r there
        if (!(fabs(t * (1.0 + tt * (th[4] + tt * (th[5] + tt * (th[6] + tt * th[7])))) - r) < kUnprojectAccept)) return false;
        const double s = sin(t) / r;
        x = mx * s; y = my * s; z = cos(t);
        return true;
    } else {
        const double k1 = th[OCV5_K1], k2 = th[OCV5_K2], p1 = th[OCV5_P1], p2 = th[OCV5_P2], k3 = th[OCV5_K3];
        double xx = mx, yy = my;
        for (int it = 0; it < 50; ++it) {
            const double q = xx * xx + yy * yy;
            const double rad = 1.0 + q * (k1 + q * (k2 + q * k3));
            const double dx = 2.0 * p1 * xx * yy + p2 * (q + 2.0 * xx * xx);
            const double dy = p1 * (q + 2.0 * yy * yy) + 2.0 * p2 * xx * yy;
            xx = (mx - dx) / rad; yy = (my - dy) / rad;
        }
        const double q = xx * xx + yy * yy, rad = 1.0 + q * (k1 + q * (k2 + q * k3));
        const double ex = xx * rad + 2.0 * p1 * xx * yy + p2 * (q + 2.0 * xx * xx) - mx;
        const double ey = yy * rad + p1 * (q + 2.0 * yy * yy) + 2.0 * p2 * xx * yy - my;
        if (!(fabs(ex) + fabs(ey) < kUnprojectAccept)) return false;
        const double n = sqrt(q + 1.0);
        x = xx / n; y = yy / n; z = 1.0 / n;
        return true;
    }
}

// Is `project` defined for this camera-frame point (the Option of GenericModel::project)?
template <int MODEL>
__device__ bool project_valid(const double* th, double x, double y, double z) {
    if constexpr (MODEL == kUCM || MODEL == kEUCM) {
        const double alpha = th[4], beta = (MODEL == kEUCM) ? th[5] : 1.0;
        const double d = sqrt(beta * (x * x + y * y) + z * z);
        const double w = alpha <= 0.5 ? alpha / (1.0 - alpha) : (1.0 - alpha) / alpha;
        return z > -w * d;
    } else if constexpr (MODEL == kKB4) {
        return x * x + y * y + z * z > 0.0;
    } else {
        return z > 1e-9;
    }
}

}  // namespace ccal

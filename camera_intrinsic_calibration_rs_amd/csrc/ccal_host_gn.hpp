// What the host-side Gauss-Newton loops of the small factors share (ccal_convert_model, ccal_init_camera_extrinsic_opts): the dense
// Cholesky factor-and-solve, the Huber weight and tiny-solver's stop rule - the host's counterpart of optimizer_decide (ccal_devopt.hpp).
// Plain C++17, no HIP include (tests/cpp/test_host_gn.cpp).  The loops stay at their call sites: masks, bounds, the start check differ.
#pragma once
#include <algorithm>
#include <cmath>

namespace ccal {

// A = L L^T in place (row-major n x n, left-looking, the lower triangle only); false: a pivot that is not a positive finite number
inline bool chol_factor(double* A, int n) {
    for (int j = 0; j < n; ++j) {
        double s = A[j * n + j];
        for (int k = 0; k < j; ++k) s -= A[j * n + k] * A[j * n + k];
        if (!(s > 0.0) || !std::isfinite(s)) return false;
        const double l = std::sqrt(s);
        A[j * n + j] = l;
        for (int i = j + 1; i < n; ++i) {
            double t = A[i * n + j];
            for (int k = 0; k < j; ++k) t -= A[i * n + k] * A[j * n + k];
            A[i * n + j] = t / l;
        }
    }
    return true;
}
// x := (L L^T)^-1 x
inline void chol_solve(const double* L, int n, double* x) {
    for (int i = 0; i < n; ++i) { double t = x[i]; for (int k = 0; k < i; ++k) t -= L[i * n + k] * x[k]; x[i] = t / L[i * n + i]; }
    for (int i = n - 1; i >= 0; --i) { double t = x[i]; for (int k = i + 1; k < n; ++k) t -= L[k * n + i] * x[k]; x[i] = t / L[i * n + i]; }
}
// HuberLoss(delta)'s corrector weight of a block with squared norm s
inline double huber_weight(double s, double delta) { return s <= delta * delta ? 1.0 : delta / std::sqrt(s); }

// tiny-solver's stop rule after a step from cost `last` to `cur`, in its order: the error below min_error, a NaN cost, the absolute and
// the relative decrease (last == 0: the quotient is inf or NaN and falls through).  error_metric: the norm, sqrt(max(cost, 0)), is read.
enum class GnNext { go_on, stop, nonfinite };
inline GnNext gn_decide(double last, double cur, int error_metric, double min_error, double min_abs, double min_rel) {
    const double le = error_metric ? std::sqrt(std::max(last, 0.0)) : last, ce = error_metric ? std::sqrt(std::max(cur, 0.0)) : cur;
    if (ce < min_error) return GnNext::stop;
    if (std::isnan(cur)) return GnNext::nonfinite;
    if (std::fabs(le - ce) < min_abs || std::fabs(le - ce) / le < min_rel) return GnNext::stop;
    return GnNext::go_on;
}

}  // namespace ccal

// What the two pose-refinement kernels share (k_pose_refine, ccal_kernels_refine.hip: one camera, one frame per wavefront;
// k_rig_pose_refine, ccal_kernels_rig_refine.hip: a rig, one frame slot per wavefront, its observations spread over cameras):
//   refine_corners   lanes stride a run of corners of ONE camera at given frame constants: residual, its 2 x 6 Jacobian w.r.t.
//                    rvec | tvec of T_0_b (corner_block<MODEL, false, OTHER>, columns P .. P + 5), the Huber corrector, lane-private
//                    lower triangle of J^T J (21), J^T r (6), the reported cost and sum rho(s) in f64 - ADDED to what the lane holds
//   refine_reduce    one xor-shuffle butterfly: the same totals on all 64 lanes, in a fixed order
//   refine_solve     (H + D) d = -g by a 6 x 6 Cholesky in registers on every lane
//   refine_lm        the Levenberg-Marquardt rule stated at ccal_refine_poses_batch (ccal.h), one state per wavefront, around a
//                    `pass` that a kernel supplies: everything between the starting pose and the result, nothing to the host between
//   RefineIO         what both argument structs end with, and the frame around the pass: refine_count / refine_min_points (the
//                    wave's valid points and what they are held against), refine_store_none / refine_store (lane 0's writes)
//   RefineResults    host: the result slices of a call's block, bound to a RefineIO; the start poses up, the seven results down
#pragma once
#include "ccal_call.hpp"
#include "ccal_device.hpp"
#include "ccal_fused.hpp"
#include "ccal_internal.hpp"

namespace ccal {

// loss, optimizer options and batch size: the tail of both kernels' argument structs
struct RefineRule {
    double delta;
    double radius0, min_diag, max_diag, min_error, min_abs, min_rel;
    int32_t n_prob, min_points, max_iter, error_metric;
};

inline RefineRule refine_rule(double huber_delta, const ccal_solver_opts* opts, int n_prob, int min_points) {      // opts NULL: the defaults
    ccal_solver_opts o;
    if (opts) o = *opts; else ccal_set_defaults(&o);
    RefineRule r;
    r.delta = huber_delta;
    r.radius0 = o.lm_initial_radius; r.min_diag = o.lm_min_diagonal; r.max_diag = o.lm_max_diagonal;
    r.min_error = o.min_error; r.min_abs = o.min_abs_error_decrease; r.min_rel = o.min_rel_error_decrease;
    r.n_prob = n_prob; r.min_points = min_points; r.max_iter = o.max_iterations; r.error_metric = o.error_metric ? 1 : 0;
    return r;
}

// what both kernels' argument structs end with (o: a problem - a frame, or a slot of a rig)
struct RefineIO {
    const double* xyz; const double* uv;     // [.][3], [.][2] pixels
    double* poses;                      // [n_prob][6] in: start, out: result
    int32_t* status; int32_t* iters; int32_t* n_used;
    double* cost0; double* cost;        // [n_prob]
    double* err;                        // [n_points] pixel error at the result, or nullptr
    RefineRule rule;
};

// The result part of a refine call's block, added where this is constructed: poses, cost0, cost | errors | status, iterations, counts
struct RefineResults {
    CallBlock& blk;
    const size_t np, n_tot;
    const Slice<double> s_res, s_err;
    const Slice<int32_t> s_int;
    RefineResults(CallBlock& b, size_t n_prob, size_t n_points, bool want_err)
        : blk(b), np(n_prob), n_tot(n_points), s_res(b.add<double>(np * 8)), s_err(b.add<double>(want_err ? n_tot + 1 : 0)), s_int(b.add<int32_t>(np * 3)) {}
    void start(RefineIO& a, const double* poses_io) const {          // after alloc() and poison(): the pointers, the start poses up
        a.poses = blk.at(s_res); a.cost0 = a.poses + np * 6; a.cost = a.poses + np * 7; a.err = blk.at(s_err);
        a.status = blk.at(s_int); a.iters = a.status + np; a.n_used = a.status + 2 * np;
        blk.upload(s_res, poses_io, np * 6);
    }
    void download(const RefineIO& a, double* poses, int32_t* status, int32_t* iters, int32_t* n_used, double* cost0, double* cost, double* err) const {
        blk.download(poses, a.poses, np * 6); blk.download(status, a.status, np); blk.download(iters, a.iters, np);
        blk.download(n_used, a.n_used, np); blk.download(cost0, a.cost0, np); blk.download(cost, a.cost, np);
        blk.download(err, a.err, n_tot);
    }
};

constexpr int kRefTri = 21;             // packed lower triangle of the 6 x 6 system: entry (i, j <= i) at i (i + 1) / 2 + j

__device__ __forceinline__ bool refine_finite(double v) { return fabs(v) < __builtin_inf(); }

__device__ __forceinline__ bool refine_point_valid(const double* xyz, const double* uv, const int c) {
    bool v = refine_finite(uv[2 * (int64_t)c]) && refine_finite(uv[2 * (int64_t)c + 1]);
#pragma unroll
    for (int k = 0; k < 3; ++k) v = v && refine_finite(xyz[3 * (int64_t)c + k]);
    return v;
}

// cnt: in, a lane's valid points; out, the wave's
__device__ __forceinline__ void refine_count(int& cnt) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
}

__device__ __forceinline__ int refine_min_points(const RefineIO& a) { return a.rule.min_points > 3 ? a.rule.min_points : 3; }   // for a result

// no result: the pose stays as the caller gave it (the NaN fill of the problem's pixel errors is the kernel's)
__device__ __forceinline__ void refine_store_none(const RefineIO& a, const int o, const int lane) {
    if (lane == 0) {
        a.status[o] = CCAL_NO_RESULT; a.iters[o] = 0; a.n_used[o] = 0; a.cost0[o] = 0.0; a.cost[o] = 0.0;
    }
}

__device__ __forceinline__ void refine_store(const RefineIO& a, const int o, const int lane, const double* pose, const int status,
                                             const int iter, const int cnt, const double cost0, const double cost) {
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) a.poses[(int64_t)o * 6 + i] = pose[i];
        a.status[o] = status; a.iters[o] = iter; a.n_used[o] = cnt;
        a.cost0[o] = cost0; a.cost[o] = cost;
    }
}

__device__ __forceinline__ void refine_zero(double* H, double* g, double& cost, double& obj) {
#pragma unroll
    for (int i = 0; i < kRefTri; ++i) H[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) g[i] = 0.0;
    cost = 0.0; obj = 0.0;
}

// The corners [0, n) of one camera at the frame constants fc (frame_setup<OTHER>): H += J^T J (packed lower), g += J^T r,
// cost += sum rho'(s) s, obj += sum rho(s), lane-private.  OTHER: the block is the OtherCamReprojectionFactor's, of which only the
// rvec_0_b | tvec_0_b columns are read - its extrinsics columns (and the frame constants only they use) are dead code.
// err != nullptr: also the pixel error of every corner (NaN for a corner that is left out).
template <int MODEL, bool OTHER>
__device__ __forceinline__ void refine_corners(const double* th, const double* fc, const double* xyz, const double* uv, double* err,
                                               const int n, const int lane, const double delta, double* H, double* g, double& cost,
                                               double& obj) {
    constexpr int P = model_np(MODEL);
    for (int c = lane; c < n; c += 64) {
        const double X = xyz[3 * (int64_t)c], Y = xyz[3 * (int64_t)c + 1], Z = xyz[3 * (int64_t)c + 2];
        const double uo = uv[2 * (int64_t)c], vo = uv[2 * (int64_t)c + 1];
        const bool valid = refine_finite(X) && refine_finite(Y) && refine_finite(Z) && refine_finite(uo) && refine_finite(vo);
        if (!valid) {
            if (err) err[c] = __builtin_nan("");
            continue;
        }
        double ru, rv, Ju[P + (OTHER ? 12 : 6)], Jv[P + (OTHER ? 12 : 6)];
        corner_block<MODEL, false, OTHER>(th, fc, X, Y, Z, uo, vo, ru, rv, Ju, Jv);
        const double s = ru * ru + rv * rv;
        if (err) err[c] = sqrt(s);
        const double sw = huber_sqrt_weight(s, delta);
        ru *= sw; rv *= sw;
        const double cs = ru * ru + rv * rv;            // rho'(s) s: s, or delta sqrt(s) for a corner beyond delta
        cost += cs;
        obj += (delta > 0.0 && s > delta * delta) ? 2.0 * cs - delta * delta : cs;      // rho(s): s, or 2 delta sqrt(s) - delta^2
        double a[6], b[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) { a[i] = sw * Ju[P + i]; b[i] = sw * Jv[P + i]; }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = 0; j <= i; ++j) H[i * (i + 1) / 2 + j] += a[i] * a[j] + b[i] * b[j];
            g[i] += a[i] * ru + b[i] * rv;
        }
    }
}

__device__ __forceinline__ void refine_reduce(double* H, double* g, double& cost, double& obj) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int i = 0; i < kRefTri; ++i) H[i] += __shfl_xor(H[i], off, 64);
#pragma unroll
        for (int i = 0; i < 6; ++i) g[i] += __shfl_xor(g[i], off, 64);
        cost += __shfl_xor(cost, off, 64);
        obj += __shfl_xor(obj, off, 64);
    }
}

// (H + diag(D)) d = -g by Cholesky, in registers (the arithmetic of chol_solve_reg).  false: not positive definite (d = 0).
__device__ __forceinline__ bool refine_solve(const double* H, const double* D, const double* g, double* d) {
    double M[kRefTri], v[6];
#pragma unroll
    for (int i = 0; i < kRefTri; ++i) M[i] = H[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) { M[i * (i + 1) / 2 + i] += D[i]; v[i] = -g[i]; }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double dj = M[j * (j + 1) / 2 + j];
#pragma unroll
        for (int k = 0; k < j; ++k) dj -= M[j * (j + 1) / 2 + k] * M[j * (j + 1) / 2 + k];
        ok = ok && (dj > 0.0) && (dj < 1.7e308);
        double sq, rs;
        fast_sqrt_rsqrt(ok ? dj : 1.0, sq, rs);
        M[j * (j + 1) / 2 + j] = rs;                       // inverted diagonal
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double t = M[i * (i + 1) / 2 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) t -= M[i * (i + 1) / 2 + k] * M[j * (j + 1) / 2 + k];
            M[i * (i + 1) / 2 + j] = t * rs;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double t = v[i];
#pragma unroll
        for (int k = 0; k < i; ++k) t -= M[i * (i + 1) / 2 + k] * v[k];
        v[i] = t * M[i * (i + 1) / 2 + i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double t = v[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) t -= M[k * (k + 1) / 2 + i] * v[k];
        v[i] = t * M[i * (i + 1) / 2 + i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) d[i] = ok ? v[i] : 0.0;
    return ok;
}

// The whole solve of one wavefront's problem from `pose` (in: the start, out: the result; wave-uniform).
//   pass(p, with_err, H, g, rep, obj): the sums over all the problem's corners at the pose p, the same on all lanes - H, g as above,
//   rep = sum rho'(s) s (reported), obj = sum rho(s) (judged); with_err: it also writes the corners' pixel errors.  It is called from
//   ONE place, once per iteration: the pass at pose + d gives the trial value and, for an accepted step, the next system.
// The rule is optimizer_decide's LM branch (ccal_fused.hpp) with the problem's own radius and stop rules.  Returns ccal_status.
template <class Pass>
__device__ __forceinline__ int refine_lm(const RefineRule& a, const bool want_err, Pass&& pass, double* pose, int& iter_out,
                                         double& cost0_out, double& cost_out) {
    double trial[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) trial[i] = pose[i];
    // cur: sum rho(s) at the accepted pose, what the steps and the stop rules are judged on; rep: the reported cost there
    double H[kRefTri], g[6], cur = 0.0, rep = 0.0, cost0 = 0.0;
    double radius = a.radius0, dec = 2.0, mc = 0.0;
    int iter = 0, done = 0;               // done: ccal_status + 1
    bool first = true, lin_ok = true, final_pass = false;
    const int em = a.error_metric;
    for (;;) {
        double Ht[kRefTri], gt[6], rt, ct;
        pass(trial, final_pass, Ht, gt, rt, ct);
        if (final_pass) break;
        bool accept = false;
        if (first) {
            first = false; accept = true; cost0 = rt;
            if (!(fabs(ct) < 1.7e308)) done = CCAL_ERR_NONFINITE + 1;
        } else {
            iter += 1;
            const double rho = (cur - ct) / mc;
            const bool fin = fabs(ct) < 1.7e308;
            const double mce = model_decrease_of(cur, mc, em);
            if (lin_ok && fin && mc >= 0.0 && (mce < a.min_abs || mce < a.min_rel * error_of(cur, em))) {
                // predicted decrease below the thresholds: converged
                accept = ct < cur;
                done = CCAL_OK + 1;
            } else if (lin_ok && fin && mc > 0.0 && rho > 0.0) {
                accept = true;
                const double t = 2.0 * rho - 1.0;
                radius = fmin(1e16, radius / fmax(1.0 / 3.0, 1.0 - t * t * t));
                dec = 2.0;
                const double le = error_of(cur, em), ce = error_of(ct, em);
                if (ce < a.min_error) done = CCAL_OK + 1;
                else if (fabs(le - ce) < a.min_abs) done = CCAL_OK + 1;
                else if (fabs(le - ce) / le < a.min_rel) done = CCAL_OK + 1;
            } else {
                radius /= dec; dec *= 2.0;
                if (radius < 1e-32) done = CCAL_ERR_NO_CONVERGENCE + 1;
            }
            if (!done && iter >= a.max_iter) done = CCAL_ERR_NO_CONVERGENCE + 1;
        }
        if (accept) {
            cur = ct; rep = rt;
#pragma unroll
            for (int i = 0; i < 6; ++i) { pose[i] = trial[i]; g[i] = gt[i]; }
#pragma unroll
            for (int i = 0; i < kRefTri; ++i) H[i] = Ht[i];
        }
        if (done) {
            if (!want_err) break;
            final_pass = true;
#pragma unroll
            for (int i = 0; i < 6; ++i) trial[i] = pose[i];
            continue;
        }
        // the damped step from the accepted point and its model decrease  d^T (D d - g)
        const double lambda = 1.0 / radius;
        double D[6], d[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) D[i] = lambda * fmin(fmax(H[i * (i + 1) / 2 + i], a.min_diag), a.max_diag);
        lin_ok = refine_solve(H, D, g, d);
        mc = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) { mc += d[i] * (D[i] * d[i] - g[i]); trial[i] = pose[i] + d[i]; }
    }
    iter_out = iter; cost0_out = cost0;
    cost_out = done == CCAL_ERR_NONFINITE + 1 ? cost0 : rep;     // (the start itself: the pose stays, the costs are what they are)
    return done - 1;
}

}  // namespace ccal

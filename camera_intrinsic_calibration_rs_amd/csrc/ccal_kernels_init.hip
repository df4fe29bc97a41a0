// Per-frame pose initialisation: what calib_camera does before it builds the
// problem -- `generic_camera.unproject(p2ds)`, keep the valid ones, divide by z, planar PnP
// (src/util.rs:418-436; the reference calls sqpnp_simple, a third-party crate).  Any PnP that lands in
// the same basin is equivalent after the joint solve; this one is the classic plane-induced homography:
//   normalised image point (xn, yn) = unproject(u, v) / z,   board point (X, Y, 0)
//   least squares for H = [h11 h12 h13; h21 h22 h23; h31 h32 1]   (8 x 8 normal equations per frame)
//   H ~ [r1 r2 t]  ->  scale, Gram-Schmidt, r3 = r1 x r2, quaternion -> rvec.
// One wavefront per observation frame; lanes own corners, 44 lane-private sums, one shuffle reduction.
#include "ccal_pose_init.hpp"

namespace ccal {

// Corners that do not span the board plane (one row, one column, a diagonal, one corner repeated) leave the design rank-deficient -
// rank 6 of 8 for a line - and no pose: rotation about the line is free.  In exact arithmetic a Cholesky pivot s is then 0; computed,
// it is a difference of at most 8 products each bounded by its diagonal entry M_jj, +-1e-16 M_jj, and its sign is rounding.  So a
// pivot is accepted on s > kPoseInitPivotTol M_jj, not on s > 0.  The two ends the tolerance sits between (tests/pose_init_cases.py
// prints them; s / M_jj does not change when board or image coordinates are rescaled):
//   from below  100 x the pivot's rounding bound 10 u = 1.1e-15, i.e. 1.1e-13 (the f64 emulation of this kernel accepted collinear
//               frames at s / M_jj = 1.7e-16; one row plus ONE corner of the next row, which exact detections leave at rank 7,
//               comes to 1.4e-14 through the f32 rounding of its detections and is refused as well);
//   from above  1 / 100 of the smallest s / M_jj of a well-posed frame of the test cases, 2.7e-6 / 100 = 2.7e-8 (a board whose
//               origin is 100 m from its corners; two adjacent rows 2.6e-3, a full board 1.6e-1).
// A frame that passes goes through exactly the arithmetic it went through under s > 0: its result keeps its bits.
constexpr double kPoseInitPivotTol = 0x1p-36;            // 1.46e-11

template <int MODEL>
__global__ __launch_bounds__(256) void k_pose_init(const InitArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int widx = blockIdx.x * WAVES_PER_BLOCK + wave;
    if (widx >= a.n_list) return;
    const int o = __builtin_amdgcn_readfirstlane(a.list[widx]);
    const int64_t start = a.obs_off[o];
    const int n = (int)(a.obs_off[o + 1] - start);
    double th[th_len<MODEL>()];
    if constexpr (MODEL == kUnprojDivision) {
#pragma unroll
        for (int i = 0; i < 5; ++i) th[i] = a.division[i];
    } else {
        load_theta<MODEL, false>(a.intr + a.cam * CCAL_PMAX, a.rt, th);
    }

    double M[36], rhs[8];            // upper triangle of A^T A (row-major packed) and A^T b
#pragma unroll
    for (int i = 0; i < 36; ++i) M[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) rhs[i] = 0.0;
    int cnt = 0, nonplanar = 0;
    for (int c = lane; c < n; c += 64) {
        const int64_t g = start + c;
        const double X = a.x[g], Y = a.y[g];
        if (a.z[g] != 0.0f) nonplanar = 1;
        double xn, yn;
        if (!unproject_normalized<MODEL>(th, a.rt.unproject_eps, (double)a.u[g], (double)a.v[g], xn, yn)) continue;
        ++cnt;
        const double r1[8] = { X, Y, 1.0, 0.0, 0.0, 0.0, -xn * X, -xn * Y };
        const double r2[8] = { 0.0, 0.0, 0.0, X, Y, 1.0, -yn * X, -yn * Y };
        int k = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int j = i; j < 8; ++j) { M[k] += r1[i] * r1[j] + r2[i] * r2[j]; ++k; }
            rhs[i] += r1[i] * xn + r2[i] * yn;
        }
    }
    // wave reduction
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int i = 0; i < 36; ++i) M[i] += __shfl_xor(M[i], off, 64);
#pragma unroll
        for (int i = 0; i < 8; ++i) rhs[i] += __shfl_xor(rhs[i], off, 64);
        cnt += __shfl_xor(cnt, off, 64);
        nonplanar |= __shfl_xor(nonplanar, off, 64);
    }
    if (lane != 0) return;
    double* out = a.poses_obs + (int64_t)o * 6;
    bool ok = cnt >= a.min_points && !nonplanar;
    // Cholesky of the 8x8 normal matrix (packed upper -> full lower), solve for h
    double L[8][8], h[8];
    if (ok) {
        int k = 0;
        for (int i = 0; i < 8; ++i) for (int j = i; j < 8; ++j) { L[j][i] = M[k]; ++k; }
        for (int j = 0; j < 8 && ok; ++j) {
            const double mjj = L[j][j];
            double s = mjj;
            for (int q = 0; q < j; ++q) s -= L[j][q] * L[j][q];
            if (!(s > kPoseInitPivotTol * mjj)) { ok = false; break; }
            const double l = sqrt(s);
            L[j][j] = l;
            for (int i = j + 1; i < 8; ++i) { double t = L[i][j]; for (int q = 0; q < j; ++q) t -= L[i][q] * L[j][q]; L[i][j] = t / l; }
        }
    }
    if (ok) {
        for (int i = 0; i < 8; ++i) { double t = rhs[i]; for (int q = 0; q < i; ++q) t -= L[i][q] * h[q]; h[i] = t / L[i][i]; }
        for (int i = 7; i >= 0; --i) { double t = h[i]; for (int q = i + 1; q < 8; ++q) t -= L[q][i] * h[q]; h[i] = t / L[i][i]; }
        // H ~ [r1 r2 t]
        double c1[3] = { h[0], h[3], h[6] }, c2[3] = { h[1], h[4], h[7] };
        const double n1 = sqrt(c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2]);
        const double n2 = sqrt(c2[0] * c2[0] + c2[1] * c2[1] + c2[2] * c2[2]);
        const double lam = 2.0 / (n1 + n2);
        double t[3] = { lam * h[2], lam * h[5], lam };
        for (int i = 0; i < 3; ++i) c1[i] /= n1;
        // h33 = 1 fixes the sign of H by the depth of the board's ORIGIN; the pose is the one with the corners in front of the
        // camera, sum_i (h31 X_i + h32 Y_i + 1) > 0 (M[2], M[9], M[15] = sum X, sum Y, n) - the rule of ccal_pnp_batch.  The
        // origin of a board may lie behind the camera's plane while its corners are in view: then [r1 r2 t] is -H, not H.
        if (h[6] * M[2] + h[7] * M[9] + M[15] < 0.0) {
            for (int i = 0; i < 3; ++i) { c1[i] = -c1[i]; c2[i] = -c2[i]; t[i] = -t[i]; }
        }
        const double d = c1[0] * c2[0] + c1[1] * c2[1] + c1[2] * c2[2];
        for (int i = 0; i < 3; ++i) c2[i] -= d * c1[i];
        const double n2b = sqrt(c2[0] * c2[0] + c2[1] * c2[1] + c2[2] * c2[2]);
        ok = n2b > 1e-12 && n1 > 1e-12 && lam == lam;
        if (ok) {
            for (int i = 0; i < 3; ++i) c2[i] /= n2b;
            const double c3[3] = { c1[1] * c2[2] - c1[2] * c2[1], c1[2] * c2[0] - c1[0] * c2[2], c1[0] * c2[1] - c1[1] * c2[0] };
            // rotation matrix R = [c1 c2 c3] (columns) -> unit quaternion (largest component first) -> rvec
            const double R00 = c1[0], R10 = c1[1], R20 = c1[2], R01 = c2[0], R11 = c2[1], R21 = c2[2], R02 = c3[0], R12 = c3[1], R22 = c3[2];
            const double tr = R00 + R11 + R22;
            double qw, qx, qy, qz;
            if (tr >= R00 && tr >= R11 && tr >= R22) {
                const double s = 2.0 * sqrt(fmax(tr + 1.0, 1e-300));
                qw = 0.25 * s; qx = (R21 - R12) / s; qy = (R02 - R20) / s; qz = (R10 - R01) / s;
            } else if (R00 >= R11 && R00 >= R22) {
                const double s = 2.0 * sqrt(fmax(1.0 + R00 - R11 - R22, 1e-300));
                qw = (R21 - R12) / s; qx = 0.25 * s; qy = (R01 + R10) / s; qz = (R02 + R20) / s;
            } else if (R11 >= R22) {
                const double s = 2.0 * sqrt(fmax(1.0 + R11 - R00 - R22, 1e-300));
                qw = (R02 - R20) / s; qx = (R01 + R10) / s; qy = 0.25 * s; qz = (R12 + R21) / s;
            } else {
                const double s = 2.0 * sqrt(fmax(1.0 + R22 - R00 - R11, 1e-300));
                qw = (R10 - R01) / s; qx = (R02 + R20) / s; qy = (R12 + R21) / s; qz = 0.25 * s;
            }
            if (qw < 0.0) { qw = -qw; qx = -qx; qy = -qy; qz = -qz; }
            const double vn = sqrt(qx * qx + qy * qy + qz * qz);
            const double ang = 2.0 * atan2(vn, qw);
            const double sc = vn > 1e-15 ? ang / vn : 0.0;
            out[0] = qx * sc; out[1] = qy * sc; out[2] = qz * sc;
            out[3] = t[0]; out[4] = t[1]; out[5] = t[2];
            ok = out[0] == out[0] && out[3] == out[3];
        }
    }
    if (!ok) for (int i = 0; i < 6; ++i) out[i] = 0.0;
    a.valid_obs[o] = ok ? cnt : 0;
}

// Frames with a corner off the z = 0 plane - k_pose_init leaves them without a pose - go to the general PnP (ccal_kernels_pnp.hip),
// which passes over every other frame; a problem without such a corner (has_nonplanar, set at creation) launches k_pose_init alone.

hipError_t launch_pose_init_division(const ccal_problem* p, int cam, double lambda, double* d_poses_obs, int32_t* d_valid, int min_points, hipStream_t s) {
    InitArgs a = pose_init_args(p, cam);
    division_theta(p, cam, lambda, a.division);
    a.poses_obs = d_poses_obs; a.valid_obs = d_valid; a.min_points = min_points; a.rt = model_rt(p->ctx);
    const int blocks = (a.n_list + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pose_init<kUnprojDivision>, dim3(blocks), dim3(256), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !p->has_nonplanar) return e;
    return launch_pose_pnp_division(p, cam, lambda, d_poses_obs, d_valid, min_points, s);
}

hipError_t launch_pose_init(const ccal_problem* p, int cam, const double* d_intr, double* d_poses_obs, int32_t* d_valid, int min_points, hipStream_t s) {
    InitArgs a = pose_init_args(p, cam);
    a.intr = d_intr; a.poses_obs = d_poses_obs; a.valid_obs = d_valid; a.min_points = min_points; a.rt = model_rt(p->ctx);
    const int blocks = (a.n_list + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    if (blocks == 0) return hipSuccess;
    switch (p->cams[cam].model) {
        case kUCM: hipLaunchKernelGGL(k_pose_init<kUCM>, dim3(blocks), dim3(256), 0, s, a); break;
        case kEUCM: hipLaunchKernelGGL(k_pose_init<kEUCM>, dim3(blocks), dim3(256), 0, s, a); break;
        case kKB4: hipLaunchKernelGGL(k_pose_init<kKB4>, dim3(blocks), dim3(256), 0, s, a); break;
        case kOCV5: hipLaunchKernelGGL(k_pose_init<kOCV5>, dim3(blocks), dim3(256), 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !p->has_nonplanar) return e;
    return launch_pose_pnp(p, cam, d_intr, d_poses_obs, d_valid, min_points, s);
}

}  // namespace ccal

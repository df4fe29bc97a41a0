// Pose initialisation for targets that are not a z = 0 plane, and the standalone batched PnP (ccal_pnp_batch): the general PnP the
// reference calls for every frame (sqpnp_simple::sqpnp_solve_glam: src/util.rs:418-436, src/optimization/linear.rs:5-21,
// examples/test_pnp.rs:61) takes any 3-D point set; k_pose_init (ccal_kernels_init.hip) is a plane-induced homography over (X, Y).
// The cost and its reduction to E(R) = vec(R)^T Omega vec(R) are in ccal_pnp.hpp.  One wavefront per frame, four per workgroup:
//   pass 1   lanes own corners: the centroid of the valid points (and, for a problem's frames, whether any z != 0)
//   pass 2   lanes own corners: the 39 centred sums, lane-private; one xor-shuffle butterfly leaves the totals on all 64 lanes
//   build    Omega (45) and P (27) on every lane, in registers (the same values in all lanes)
//   refine   lane l starts at rotation l of a fixed table of 64 well-spread rotations: kPnpIters damped Gauss-Newton steps, the
//            same count on every lane
//   select   wave arg-min over (in front of the camera, cost, lane): ties go to the lowest lane; the winning lane writes
// A frame gets no pose - six zeros, n_used 0 - with fewer than max(min_points, 4) valid points, a singular sum Q^T Q, collinear
// points (second eigenvalue of the centred scatter <= kPnpCollinearRel x the largest), no candidate in front of the camera
// (sum_i (R X_i + t)_z = n t'_z <= 0 for all 64, or the candidates behind it fit so much better that the points lie behind the
// camera: pnp_points_behind), or a result that is not finite.  Every output element of a frame this kernel
// takes is written on every path.
#include "ccal_pnp.hpp"
#include "ccal_pose_init.hpp"

namespace ccal {

constexpr int kPnpDirect = 101;          // not a camera model: points and normalised image points as given (ccal_pnp_batch)

__constant__ double kPnpStartTab[kPnpStarts][4] = { CCAL_PNP_START_TABLE };

struct PnpArgs {
    InitArgs init;                        // a problem's frames (MODEL != kPnpDirect); poses_obs / valid_obs / min_points for both
    const double* xyz; const double* xn;  // kPnpDirect: [.][3], [.][2]
    const int64_t* off; int32_t n_prob;   // kPnpDirect: [n_prob + 1]
    double* cost;                         // kPnpDirect: [n_prob] E at the result (0 without one), or nullptr
};

template <int MODEL>
__global__ __launch_bounds__(256) void k_pose_pnp(const PnpArgs a) {
    constexpr bool kDirect = MODEL == kPnpDirect;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int widx = blockIdx.x * WAVES_PER_BLOCK + wave;
    if (widx >= (kDirect ? a.n_prob : a.init.n_list)) return;
    int o = widx;
    if constexpr (!kDirect) o = __builtin_amdgcn_readfirstlane(a.init.list[widx]);
    const int64_t* offs = kDirect ? a.off : a.init.obs_off;
    const int64_t start = offs[o];
    const int n = (int)(offs[o + 1] - start);
    double th[th_len<MODEL>()];
    if constexpr (MODEL == kUnprojDivision) {
#pragma unroll
        for (int i = 0; i < 5; ++i) th[i] = a.init.division[i];
    } else if constexpr (!kDirect) {
        load_theta<MODEL, false>(a.init.intr + a.init.cam * CCAL_PMAX, a.init.rt, th);
    }
    // corner g of the frame: board point and normalised image point; false: no ray (or, given directly, not finite)
    auto point = [&](int64_t g, double& X, double& Y, double& Z, double& xn, double& yn) -> bool {
        if constexpr (kDirect) {
            X = a.xyz[3 * g]; Y = a.xyz[3 * g + 1]; Z = a.xyz[3 * g + 2]; xn = a.xn[2 * g]; yn = a.xn[2 * g + 1];
            return fabs(X) < 1e300 && fabs(Y) < 1e300 && fabs(Z) < 1e300 && fabs(xn) < 1e300 && fabs(yn) < 1e300;
        } else {
            X = a.init.x[g]; Y = a.init.y[g]; Z = a.init.z[g];
            return unproject_normalized<MODEL>(th, a.init.rt.unproject_eps, (double)a.init.u[g], (double)a.init.v[g], xn, yn);
        }
    };

    // pass 1: centroid of the valid points
    double cen[3] = { 0.0, 0.0, 0.0 };
    int cnt = 0, nonplanar = 0;
    for (int c = lane; c < n; c += 64) {
        double X, Y, Z, xn, yn;
        const bool v = point(start + c, X, Y, Z, xn, yn);
        if (Z != 0.0) nonplanar = 1;
        if (!v) continue;
        ++cnt; cen[0] += X; cen[1] += Y; cen[2] += Z;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int i = 0; i < 3; ++i) cen[i] += __shfl_xor(cen[i], off, 64);
        cnt += __shfl_xor(cnt, off, 64);
        nonplanar |= __shfl_xor(nonplanar, off, 64);
    }
    if (!kDirect && !nonplanar) return;          // every z == 0: k_pose_init's frame, its outputs stay as that kernel wrote them
    double* out = a.init.poses_obs + (int64_t)o * 6;
    bool ok = cnt >= (a.init.min_points > 4 ? a.init.min_points : 4);
    int best = kPnpStarts;
    double E = 0.0, q[4] = { 1.0, 0.0, 0.0, 0.0 }, P[27], tr_om = 0.0;
    if (ok) {                                    // (the same on all lanes, like every branch up to the winner's)
#pragma unroll
        for (int i = 0; i < 3; ++i) cen[i] /= (double)cnt;
        // pass 2: the centred sums
        double s[kPnpNSums];
#pragma unroll
        for (int i = 0; i < kPnpNSums; ++i) s[i] = 0.0;
        for (int c = lane; c < n; c += 64) {
            double X, Y, Z, xn, yn;
            if (!point(start + c, X, Y, Z, xn, yn)) continue;
            pnp_accumulate(s, X - cen[0], Y - cen[1], Z - cen[2], xn, yn);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int i = 0; i < kPnpNSums; ++i) s[i] += __shfl_xor(s[i], off, 64);
        }
        double Om[45];
        ok = pnp_build(s, cnt, Om, P);
        tr_om = pnp_trace(Om);
        if (ok) {
#pragma unroll
            for (int i = 0; i < 4; ++i) q[i] = kPnpStartTab[lane][i];
            E = pnp_refine(Om, q);
        }
    }
    double R[9], tc[3];
    pnp_quat_to_R(q, R);
    if (ok) {
        pnp_centroid_position(P, R, tc);
        const bool front = tc[2] > 0.0 && E < 1e300;                 // (false for a NaN cost)
        double bE = front ? E : __builtin_inf();
        double behindE = (tc[2] < 0.0 && E < 1e300) ? E : __builtin_inf();      // the lowest cost behind the camera
        best = front ? lane : kPnpStarts;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double oE = __shfl_xor(bE, off, 64);
            const int ol = __shfl_xor(best, off, 64);
            const bool take = oE < bE || (oE == bE && ol < best);
            bE = take ? oE : bE; best = take ? ol : best;
            behindE = fmin(behindE, __shfl_xor(behindE, off, 64));
        }
        if (pnp_points_behind(bE, behindE, tr_om)) best = kPnpStarts;      // the frame's points lie behind the camera (ccal_pnp.hpp)
    }
    if (best == kPnpStarts) {                    // no pose
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 6; ++i) out[i] = 0.0;
            a.init.valid_obs[o] = 0;
            if (kDirect && a.cost) a.cost[o] = 0.0;
        }
        return;
    }
    if (lane != best) return;
    double pose[6];
    const bool fin = pnp_pose(q, R, tc, cen, pose);
#pragma unroll
    for (int i = 0; i < 6; ++i) out[i] = fin ? pose[i] : 0.0;
    a.init.valid_obs[o] = fin ? cnt : 0;
    if (kDirect && a.cost) a.cost[o] = fin && E > 0.0 ? E : 0.0;       // (a sum of squares: rounding of the quadratic form may leave -1e-15)
}

template <int MODEL>
static hipError_t launch_pnp(const PnpArgs& a, int n_frames, hipStream_t s) {
    const int blocks = (n_frames + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pose_pnp<MODEL>, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

// the frames of camera `cam` with any z != 0 (k_pose_init, launched before on the same stream, left them without a pose)
hipError_t launch_pose_pnp(const ccal_problem* p, int cam, const double* d_intr, double* d_poses_obs, int32_t* d_valid, int min_points, hipStream_t s) {
    PnpArgs a = {};
    a.init = pose_init_args(p, cam);
    a.init.intr = d_intr; a.init.poses_obs = d_poses_obs; a.init.valid_obs = d_valid; a.init.min_points = min_points; a.init.rt = model_rt(p->ctx);
    switch (p->cams[cam].model) {
        case kUCM: return launch_pnp<kUCM>(a, a.init.n_list, s);
        case kEUCM: return launch_pnp<kEUCM>(a, a.init.n_list, s);
        case kKB4: return launch_pnp<kKB4>(a, a.init.n_list, s);
        case kOCV5: return launch_pnp<kOCV5>(a, a.init.n_list, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_pose_pnp_division(const ccal_problem* p, int cam, double lambda, double* d_poses_obs, int32_t* d_valid, int min_points, hipStream_t s) {
    PnpArgs a = {};
    a.init = pose_init_args(p, cam);
    division_theta(p, cam, lambda, a.init.division);
    a.init.poses_obs = d_poses_obs; a.init.valid_obs = d_valid; a.init.min_points = min_points; a.init.rt = model_rt(p->ctx);
    return launch_pnp<kUnprojDivision>(a, a.init.n_list, s);
}

hipError_t launch_pnp_batch(int n_prob, const int64_t* d_off, const double* d_xyz, const double* d_xn, int min_points,
                            double* d_poses, int32_t* d_n_used, double* d_cost, hipStream_t s) {
    PnpArgs a = {};
    a.xyz = d_xyz; a.xn = d_xn; a.off = d_off; a.n_prob = n_prob; a.cost = d_cost;
    a.init.poses_obs = d_poses; a.init.valid_obs = d_n_used; a.init.min_points = min_points;
    return launch_pnp<kPnpDirect>(a, n_prob, s);
}

}  // namespace ccal

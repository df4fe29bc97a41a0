// The general PnP behind the pose initialisation of non-planar targets (ccal_kernels_pnp.hip): the cost SQPnP is built on
// (Terzakis & Lourakis, ECCV 2020).  For board points X_i and normalised image points (x_i, y_i):
//   e_i(R, t) = Q_i (R X_i + t),  Q_i = [1 0 -x_i; 0 1 -y_i],  E(R, t) = sum |e_i|^2
//   E is quadratic in t:  t*(R) = P vec(R),  P = -(sum Q^T Q)^-1 sum Q^T Q A_i,  A_i = kron(I3, X_i^T)  (vec = row-major)
//   E(R) = vec(R)^T Omega vec(R),  Omega = sum A^T Q^T Q A + (sum A^T Q^T Q) P   (9 x 9, symmetric, PSD)
// The X_i are centred on their centroid before the sums (t' = t + R centroid is what P gives), so sum_i (R X_i + t)_z = n t'_z.
// Everything here is plain scalar C++ with compile-time array indices (no scratch memory on the device), shared by the kernel
// and by host-side checks.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CCAL_PNP_FN __host__ __device__ __forceinline__
#else
#define CCAL_PNP_FN inline
#endif

namespace ccal {

constexpr int kPnpStarts = 64;              // one per lane of a wavefront
constexpr int kPnpIters = 24;               // damped Gauss-Newton steps from every start (the same count on every lane)
constexpr int kPnpPolish = 2;               // undamped steps behind them, taken wherever they are short (see pnp_refine)
constexpr double kPnpCollinearRel = 1e-6;   // no pose unless the second eigenvalue of the centred scatter exceeds this x the largest
constexpr double kPnpSingularRel = 1e-12;   // no pose unless det(sum Q^T Q) / n = n sq - sx^2 - sy^2 exceeds this x n sq

// A frame whose points lie BEHIND the camera has its global minimum of E at negative depth, and the best candidate in front of
// the camera is some other, poor local minimum of E.  For points in front it is the other way round; a coplanar target's mirror
// twin ties, and with a handful of noisy, nearly coplanar points either of the two may come out lower by chance.  So: no pose when
// the lowest cost among the candidates behind the camera is below kPnpBehindRatio x the lowest in front, less kPnpBehindFloorRel x
// trace(Omega).  trace(Omega) / 3 is the mean of E over all rotations, the scale of a fit that explains nothing: the floor keeps
// the rule away from frames whose best pose in front fits to better than 1e-4 of that scale (measurement noise, rounding), where
// the two costs say nothing about the side of the camera.
constexpr double kPnpBehindRatio = 0.5;
constexpr double kPnpBehindFloorRel = 5e-5;

// The per-frame sums (over the valid points, X centred), flat so that one loop reduces them:
//   S0 = sum X X^T, Sx = sum x X X^T, Sy = sum y X X^T, Sq = sum (x^2 + y^2) X X^T     (packed 00 01 02 11 12 22)
//   V1 = sum X, Vx = sum x X, Vy = sum y X, Vq = sum (x^2 + y^2) X;  sx = sum x, sy = sum y, sq = sum (x^2 + y^2)
constexpr int kPnpS0 = 0, kPnpSx = 6, kPnpSy = 12, kPnpSq = 18, kPnpV1 = 24, kPnpVx = 27, kPnpVy = 30, kPnpVq = 33, kPnpSc = 36, kPnpNSums = 39;

CCAL_PNP_FN void pnp_accumulate(double (&s)[kPnpNSums], double X, double Y, double Z, double x, double y) {
    const double q = x * x + y * y;
    const double xx[6] = { X * X, X * Y, X * Z, Y * Y, Y * Z, Z * Z };
    const double v[3] = { X, Y, Z };
#pragma unroll
    for (int i = 0; i < 6; ++i) { s[kPnpS0 + i] += xx[i]; s[kPnpSx + i] += x * xx[i]; s[kPnpSy + i] += y * xx[i]; s[kPnpSq + i] += q * xx[i]; }
#pragma unroll
    for (int i = 0; i < 3; ++i) { s[kPnpV1 + i] += v[i]; s[kPnpVx + i] += x * v[i]; s[kPnpVy + i] += y * v[i]; s[kPnpVq + i] += q * v[i]; }
    s[kPnpSc] += x; s[kPnpSc + 1] += y; s[kPnpSc + 2] += q;
}

// packed upper triangle of a symmetric 9 x 9 (row-major): 45 entries
constexpr int pnp_sym9(int i, int j) { return i <= j ? i * 9 - i * (i - 1) / 2 + (j - i) : j * 9 - j * (j - 1) / 2 + (i - j); }
constexpr int pnp_sym3(int i, int j) { return i <= j ? i * 3 - i * (i - 1) / 2 + (j - i) : j * 3 - j * (j - 1) / 2 + (i - j); }

// Second-largest over largest eigenvalue of a symmetric PSD 3 x 3 (packed), by the trigonometric closed form; 0 for the zero matrix.
CCAL_PNP_FN double pnp_scatter_ratio(const double* a) {
    const double p1 = a[1] * a[1] + a[2] * a[2] + a[4] * a[4];
    const double qm = (a[0] + a[3] + a[5]) / 3.0;
    const double d0 = a[0] - qm, d1 = a[3] - qm, d2 = a[5] - qm;
    const double p = std::sqrt((d0 * d0 + d1 * d1 + d2 * d2 + 2.0 * p1) / 6.0);
    if (!(qm > 0.0)) return 0.0;
    if (!(p > 1e-300)) return 1.0;                                     // a multiple of the identity
    const double b00 = d0 / p, b11 = d1 / p, b22 = d2 / p, b01 = a[1] / p, b02 = a[2] / p, b12 = a[4] / p;
    double r = 0.5 * (b00 * (b11 * b22 - b12 * b12) - b01 * (b01 * b22 - b12 * b02) + b02 * (b01 * b12 - b11 * b02));
    r = r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r);
    const double phi = std::acos(r) / 3.0;
    const double e1 = qm + 2.0 * p * std::cos(phi);
    const double e3 = qm + 2.0 * p * std::cos(phi + 2.0943951023931954923);
    const double e2 = 3.0 * qm - e1 - e3;
    return e1 > 0.0 ? e2 / e1 : 0.0;
}

// Omega (packed, 45) and P (3 x 9, row-major) from the sums of n points.  false: sum Q^T Q is singular or the points are collinear.
CCAL_PNP_FN bool pnp_build(const double (&s)[kPnpNSums], int n, double (&Om)[45], double (&P)[27]) {
    const double a = (double)n, sx = s[kPnpSc], sy = s[kPnpSc + 1], sq = s[kPnpSc + 2];
    const double dn = a * sq - sx * sx - sy * sy;                       // det(sum Q^T Q) = n dn
    bool ok = dn > kPnpSingularRel * a * sq;
    ok = ok && pnp_scatter_ratio(&s[kPnpS0]) > kPnpCollinearRel;
    const double idet = 1.0 / (a * dn);
    // inverse of [[a, 0, -sx], [0, a, -sy], [-sx, -sy, sq]] (packed symmetric)
    const double Mi[6] = { (a * sq - sy * sy) * idet, sx * sy * idet, a * sx * idet, (a * sq - sx * sx) * idet, a * sy * idet, a * a * idet };
    // B = sum Q^T Q A (3 x 9): [V1 0 -Vx; 0 V1 -Vy; -Vx -Vy Vq]
    double B[3][9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        B[0][k] = s[kPnpV1 + k]; B[0][3 + k] = 0.0; B[0][6 + k] = -s[kPnpVx + k];
        B[1][k] = 0.0; B[1][3 + k] = s[kPnpV1 + k]; B[1][6 + k] = -s[kPnpVy + k];
        B[2][k] = -s[kPnpVx + k]; B[2][3 + k] = -s[kPnpVy + k]; B[2][6 + k] = s[kPnpVq + k];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 9; ++c)
            P[r * 9 + c] = -(Mi[pnp_sym3(r, 0)] * B[0][c] + Mi[pnp_sym3(r, 1)] * B[1][c] + Mi[pnp_sym3(r, 2)] * B[2][c]);
    // Omega = blocks [S0 0 -Sx; 0 S0 -Sy; -Sx -Sy Sq] + B^T P
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int j = i; j < 9; ++j) {
            const int bi = i / 3, bj = j / 3, e = pnp_sym3(i % 3, j % 3);
            double raw = 0.0;
            if (bi == bj) raw = bi == 2 ? s[kPnpSq + e] : s[kPnpS0 + e];
            else if (bj == 2) raw = bi == 0 ? -s[kPnpSx + e] : -s[kPnpSy + e];
            Om[pnp_sym9(i, j)] = raw + B[0][i] * P[j] + B[1][i] * P[9 + j] + B[2][i] * P[18 + j];
        }
    return ok;
}

CCAL_PNP_FN void pnp_symv9(const double (&Om)[45], const double (&v)[9], double (&o)[9]) {
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        double t = 0.0;
#pragma unroll
        for (int j = 0; j < 9; ++j) t += Om[pnp_sym9(i, j)] * v[j];
        o[i] = t;
    }
}
CCAL_PNP_FN double pnp_dot9(const double (&a)[9], const double (&b)[9]) {
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) t += a[i] * b[i];
    return t;
}

// unit quaternion (w, x, y, z) -> rotation matrix, row-major
CCAL_PNP_FN void pnp_quat_to_R(const double (&q)[4], double (&R)[9]) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z); R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z); R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y); R[7] = 2.0 * (y * z + w * x); R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// kPnpIters damped Gauss-Newton steps on E(R) = vec(R)^T Omega vec(R) over the three rotation coordinates w of exp(w^) R, from
// the unit quaternion q.  Each step: the 9 x 3 Jacobian of vec(exp(w^) R) at w = 0 (columns [0; -r2; r1], [r2; 0; -r0],
// [-r1; r0; 0] of R's rows), (J^T Omega J + d I) w = -J^T Omega vec(R), R <- R(normalise((1, w / 2) * q)) (the exponential to
// second order, exactly a rotation); the step is kept only where E decreases, the damping follows (x 0.1 / x 10).  Comparing two
// costs resolves a minimum only to the square root of the rounding of E, so kPnpPolish undamped steps follow that are kept wherever
// they are short (|w / 2|^2 < 1e-10: a converged candidate) - the zero of the gradient J^T Omega vec(R), which rounding leaves far
// sharper.  No branch depends on the data.  Returns E at the quaternion left in q.
CCAL_PNP_FN double pnp_refine(const double (&Om)[45], double (&q)[4]) {
    double R[9], W[9];
    pnp_quat_to_R(q, R);
    pnp_symv9(Om, R, W);
    double E = pnp_dot9(R, W), mu = 1e-3;
    for (int it = 0; it < kPnpIters + kPnpPolish; ++it) {
        const bool polish = it >= kPnpIters;
        const double Jx[9] = { 0.0, 0.0, 0.0, -R[6], -R[7], -R[8], R[3], R[4], R[5] };
        const double Jy[9] = { R[6], R[7], R[8], 0.0, 0.0, 0.0, -R[0], -R[1], -R[2] };
        const double Jz[9] = { -R[3], -R[4], -R[5], R[0], R[1], R[2], 0.0, 0.0, 0.0 };
        double Mx[9], My[9], Mz[9];
        pnp_symv9(Om, Jx, Mx); pnp_symv9(Om, Jy, My); pnp_symv9(Om, Jz, Mz);
        const double hxy = pnp_dot9(Jx, My), hxz = pnp_dot9(Jx, Mz), hyz = pnp_dot9(Jy, Mz);
        const double tx = pnp_dot9(Jx, Mx), ty = pnp_dot9(Jy, My), tz = pnp_dot9(Jz, Mz);
        const double gx = pnp_dot9(Jx, W), gy = pnp_dot9(Jy, W), gz = pnp_dot9(Jz, W);
        const double d = (polish ? 0.0 : mu) * (tx + ty + tz) * (1.0 / 3.0) + 1e-300;
        const double hxx = tx + d, hyy = ty + d, hzz = tz + d;
        const double c0 = hyy * hzz - hyz * hyz, c1 = hxz * hyz - hxy * hzz, c2 = hxy * hyz - hxz * hyy;
        const double det = hxx * c0 + hxy * c1 + hxz * c2;
        const double id = det > 0.0 ? -0.5 / det : 0.0;                  // (w / 2, and the minus of -g)
        const double wx = id * (c0 * gx + c1 * gy + c2 * gz);
        const double wy = id * (c1 * gx + (hxx * hzz - hxz * hxz) * gy + (hxz * hxy - hxx * hyz) * gz);
        const double wz = id * (c2 * gx + (hxz * hxy - hxx * hyz) * gy + (hxx * hyy - hxy * hxy) * gz);
        // (1, wx, wy, wz) * q, normalised
        double qn[4] = { q[0] - wx * q[1] - wy * q[2] - wz * q[3], q[1] + wx * q[0] + wy * q[3] - wz * q[2],
                         q[2] - wx * q[3] + wy * q[0] + wz * q[1], q[3] + wx * q[2] - wy * q[1] + wz * q[0] };
        const double inv = 1.0 / std::sqrt(qn[0] * qn[0] + qn[1] * qn[1] + qn[2] * qn[2] + qn[3] * qn[3]);
#pragma unroll
        for (int i = 0; i < 4; ++i) qn[i] *= inv;
        double Rn[9], Wn[9];
        pnp_quat_to_R(qn, Rn);
        pnp_symv9(Om, Rn, Wn);
        const double En = pnp_dot9(Rn, Wn);
        const bool acc = polish ? (wx * wx + wy * wy + wz * wz < 1e-10 && En < 1e300) : En < E;
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = acc ? qn[i] : q[i];
#pragma unroll
        for (int i = 0; i < 9; ++i) { R[i] = acc ? Rn[i] : R[i]; W[i] = acc ? Wn[i] : W[i]; }
        E = acc ? En : E;
        mu = acc ? (mu > 1e-8 ? mu * 0.1 : 1e-9) : (mu < 1e8 ? mu * 10.0 : 1e9);
    }
    return E;
}

CCAL_PNP_FN double pnp_trace(const double (&Om)[45]) {
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) t += Om[pnp_sym9(i, i)];
    return t;
}
// the rule above: best_front / best_behind = the lowest E among the candidates with t'_z > 0 / t'_z < 0 (+inf: none)
CCAL_PNP_FN bool pnp_points_behind(double best_front, double best_behind, double trace_om) {
    return best_behind < kPnpBehindRatio * best_front - kPnpBehindFloorRel * trace_om;
}

// The pose of a refined candidate: t' = P vec(R) (the centroid's position; in front of the camera iff t'_z > 0), t = t' - R centroid,
// rvec from the quaternion with qw >= 0.  false: not finite.
CCAL_PNP_FN void pnp_centroid_position(const double (&P)[27], const double (&R)[9], double (&tc)[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < 9; ++c) t += P[r * 9 + c] * R[c];
        tc[r] = t;
    }
}
CCAL_PNP_FN bool pnp_pose(const double (&q)[4], const double (&R)[9], const double (&tc)[3], const double (&cen)[3], double (&pose)[6]) {
    double qw = q[0], qx = q[1], qy = q[2], qz = q[3];
    if (qw < 0.0) { qw = -qw; qx = -qx; qy = -qy; qz = -qz; }
    const double vn = std::sqrt(qx * qx + qy * qy + qz * qz);
    const double ang = 2.0 * std::atan2(vn, qw);
    const double sc = vn > 1e-15 ? ang / vn : 0.0;
    pose[0] = qx * sc; pose[1] = qy * sc; pose[2] = qz * sc;
#pragma unroll
    for (int r = 0; r < 3; ++r) pose[3 + r] = tc[r] - (R[3 * r] * cen[0] + R[3 * r + 1] * cen[1] + R[3 * r + 2] * cen[2]);
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) fin = fin && std::fabs(pose[i]) < 1e300;       // false for NaN and infinity
    return fin;
}

// The 64 starting rotations, (w, x, y, z): the super-Fibonacci spiral on SO(3) (Alexa, CVPR 2022) for n = 64,
//   s = i + 1/2, q_i = (sqrt(1 - s/n) cos(2 pi s / psi), sqrt(s/n) sin(2 pi s / sqrt 2), sqrt(s/n) cos(2 pi s / sqrt 2), sqrt(1 - s/n) sin(2 pi s / psi)),
//   psi = 1.533751168755204288 - every rotation lies within 60 degrees of one of them.
#define CCAL_PNP_START_TABLE \
    { -0.45777066556297641, 0.070330007321550023, -0.053536810421902434, 0.88466576612301984 }, \
    { 0.97878081554824448, 0.056947279261425517, 0.14210737976868484, -0.13620064285719638 }, \
    { -0.6710860322861939, -0.19641212860204452, 0.022017623350714496, -0.71454953451134073 }, \
    { -0.19409367855984247, 0.036765993181816593, -0.23094536528225595, 0.95270149781718549 }, \
    { 0.88243704952923996, 0.24131483510794047, 0.10990746269852426, -0.38857734573457814 }, \
    { -0.81991606293622643, -0.18815372256708973, 0.2248014161079655, -0.49173178638273729 }, \
    { 0.071544240184099814, -0.18110211965904049, -0.26222990343399549, 0.94515550133111959 }, \
    { 0.72385358113622966, 0.32330811484892197, -0.11251383413979056, -0.59903964232449258 }, \
    { -0.89904012203399153, 0.02381453133495012, 0.36365556244514763, -0.24272280274647814 }, \
    { 0.31823123434773198, -0.37727800320783267, -0.078094867280190772, 0.86619361662709049 }, \
    { 0.51846519617080633, 0.18474560689271044, -0.36046020686595093, -0.7530812309170688 }, \
    { -0.90563641264627615, 0.31213885320678653, 0.2868045263219397, 0.011627041291054333 }, \
    { 0.52748319945735733, -0.37486747056446657, 0.23406597256457165, 0.72556803560398786 }, \
    { 0.28482350191271288, -0.13074175999626667, -0.44027729011735167, -0.84139055899040061 }, \
    { -0.84288897671913299, 0.47589851521693943, -0.009116096440502373, 0.25094954258849128 }, \
    { 0.68467990534529433, -0.12192202990060928, 0.47678351337364316, 0.53761131611635449 }, \
    { 0.042950516189264196, -0.44067287063356625, -0.25222989729128525, -0.86043172486785713 }, \
    { -0.71950487387411899, 0.37121880228504189, -0.36828535245113819, 0.45702870420947106 }, \
    { 0.78013812552406769, 0.26336916169162949, 0.46872079607144412, 0.31987810976025538 }, \
    { -0.18738309282713608, -0.53584504093307428, 0.13250506445955976, -0.8125269697201053 }, \
    { -0.5487835934928641, 0.015328169143535882, -0.56575396351303375, 0.61524309627419538 }, \
    { 0.80974072479692794, 0.55429452270239454, 0.16939622812248384, 0.09155576773391122 }, \
    { -0.38830984107151206, -0.31801259419746547, 0.50043030476960348, -0.70544522631244522 }, \
    { -0.34732652784992557, -0.40643504668767721, -0.44944193487477974, 0.71566527305138605 }, \
    { 0.77507910405725977, 0.55283357655674403, -0.27782645056127858, -0.12821810501561592 }, \
    { -0.54531063518652989, 0.1230393912375591, 0.61911130518178303, -0.55154221157810157 }, \
    { -0.13350266632513852, -0.64174773638515226, -0.04714173145455347, 0.75373373155516854 }, \
    { 0.68310781082939376, 0.22035230243447848, -0.61735918460149608, -0.3219879171395616 }, \
    { -0.64833648960740498, 0.54606982042194641, 0.38356257797697541, -0.36653416790736904 }, \
    { 0.074195110876855541, -0.52407007013793971, 0.43161100725724677, 0.7304502621821497 }, \
    { 0.54535104565572046, -0.28114177895958703, -0.63049329903135276, -0.47542584805857185 }, \
    { -0.69251926044148004, 0.69368933390183507, -0.10479793905811512, -0.16801658822147733 }, \
    { 0.25876207674394053, -0.085001423318725233, 0.70752191346543536, 0.65209637910293838 }, \
    { 0.37673786007022736, -0.66941707706271758, -0.27444175508986901, -0.57847306314962132 }, \
    { -0.67842032320450318, 0.44933090299639145, -0.58065845349262557, 0.026141252133313645 }, \
    { 0.40612631081633027, 0.44639354490077165, 0.59617137055625435, 0.52950346520369207 }, \
    { 0.19417305087667816, -0.70320561240645041, 0.27534408778847785, -0.62608651663587434 }, \
    { -0.61180662981122791, -0.079236234621576515, -0.76135347843363432, 0.19938692965946181 }, \
    { 0.50630713225603174, 0.76496762380471206, 0.12801185308623797, 0.37694905203047419 }, \
    { 0.014971742125979468, -0.33128806824476392, 0.71234522237371167, -0.61853726398472808 }, \
    { -0.50298505140844774, -0.6059517898450324, -0.51539783505909464, 0.33792534391436407 }, \
    { 0.55419566331799397, 0.66620671100695039, -0.45233407809859061, 0.21078345940687265 }, \
    { -0.1447040641101516, 0.26172228207588039, 0.77172789703689826, -0.56124703458459824 }, \
    { -0.36576553410271789, -0.82307102208854666, 0.047345460163728044, 0.43188896033882779 }, \
    { 0.5499014980604966, 0.17549369075540783, -0.81517756624249993, 0.047914949972025181 }, \
    { -0.27126937058284334, 0.74728311360047994, 0.39051945934559057, -0.46419330949895005 }, \
    { -0.21615968215839121, -0.58167942799977579, 0.62306624290026635, 0.47614335216317288 }, \
    { 0.49865171849281115, -0.45046685378183732, -0.73434808751973535, -0.095702474597923706 }, \
    { -0.35487300624508811, 0.83644726905826849, -0.24118139663946833, -0.34095842772774171 }, \
    { -0.070955353079564076, 0.0098669803582504701, 0.87939760216787599, 0.47066743871799166 }, \
    { 0.41027711486008639, -0.85882646186201816, -0.22689118185942667, -0.20642235591641597 }, \
    { -0.39017391353444303, 0.45177579233748094, -0.77497492440584248, -0.20754955359435734 }, \
    { 0.053649339596375405, 0.63276790901263225, 0.64801024168124177, 0.42048691818042666 }, \
    { 0.29838127338983461, -0.80061422021731921, 0.44153637492942061, -0.27391808207977214 }, \
    { -0.37662259977089219, -0.21440635468875824, -0.8975480015403513, -0.081196781597636783 }, \
    { 0.14306929092969556, 0.93065804734805335, 0.032605197535185954, 0.3351770845282746 }, \
    { 0.17939256237493836, -0.28172518274406255, 0.89635005517254507, -0.29155755617811357 }, \
    { -0.3180324073025072, -0.79593478222873637, -0.51470896867889748, 0.020442306752716785 }, \
    { 0.18432329196860325, 0.71418159379589885, -0.63561556862867175, 0.22795267938293037 }, \
    { 0.072018961599385201, 0.42611274441533886, 0.86493666187000551, -0.25519751011745057 }, \
    { -0.22041034440984997, -0.95509567587749034, 0.18194710747939913, 0.078145889700811058 }, \
    { 0.16150875603676162, 0.079569606795489689, -0.97703949647617183, 0.11391848718912054 }, \
    { -0.00022585819759143297, 0.92803926382208912, 0.33956681935158955, -0.15309294231960721 }, \
    { -0.072078276324246765, -0.57898173133454534, 0.81053541241629434, 0.051158792813411152 },

}  // namespace ccal

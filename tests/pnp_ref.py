"""numpy f64 yardstick for the general PnP (ccal_pnp_batch, csrc/ccal_kernels_pnp.hip), written independently of the kernel.

The cost is the one SQPnP is built on: e_i(R, t) = Q_i (R X_i + t) with Q_i = [1 0 -x_i; 0 1 -y_i], E = sum |e_i|^2, quadratic in t,
so t*(R) = P vec(R) and E(R) = vec(R)^T Omega vec(R) (vec = row-major; the X_i centred on their centroid first).  Here Omega and P
come from explicit per-point matrices, the minimiser from 512 seeded random rotations, each refined by Levenberg-Marquardt on so(3)
(true exponential map) until its step stalls or 200 iterations; the lowest cost with positive summed depth wins.
"""
import numpy as np

from camera_intrinsic_calibration_rs_amd import synth

N_STARTS = 512


def omega_p(X, xn):
    """X [n, 3], xn [n, 2] -> (Omega [9, 9], P [3, 9], centroid [3]); t = P vec(R) - R centroid."""
    X = np.asarray(X, dtype=np.float64); xn = np.asarray(xn, dtype=np.float64)
    n = X.shape[0]
    cen = X.mean(axis=0)
    Xc = X - cen
    A = np.zeros((n, 3, 9))
    for r in range(3):
        A[:, r, 3 * r:3 * r + 3] = Xc
    Q = np.zeros((n, 2, 3))
    Q[:, 0, 0] = 1.0; Q[:, 1, 1] = 1.0; Q[:, 0, 2] = -xn[:, 0]; Q[:, 1, 2] = -xn[:, 1]
    QQ = np.einsum("nki,nkj->nij", Q, Q)
    M = QQ.sum(axis=0)
    B = np.einsum("nij,njk->ik", QQ, A)
    P = -np.linalg.solve(M, B)
    Om = np.einsum("nji,njk,nkl->il", A, QQ, A) + B.T @ P
    return 0.5 * (Om + Om.T), P, cen


def cost(X, xn, R, t):
    """E recomputed from the definition (no Omega): sum over points of |Q_i (R X_i + t)|^2."""
    pc = np.asarray(X, dtype=np.float64) @ np.asarray(R).T + np.asarray(t)
    xn = np.asarray(xn, dtype=np.float64)
    return float(((pc[:, 0] - xn[:, 0] * pc[:, 2]) ** 2 + (pc[:, 1] - xn[:, 1] * pc[:, 2]) ** 2).sum())


def _random_rotations(seed, n):
    q = synth.normal01(seed, 4 * n, stream=21).reshape(n, 4)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)


_GEN = np.zeros((3, 3, 3))
_GEN[0, 1, 2], _GEN[0, 2, 1] = -1.0, 1.0
_GEN[1, 0, 2], _GEN[1, 2, 0] = 1.0, -1.0
_GEN[2, 0, 1], _GEN[2, 1, 0] = -1.0, 1.0


def _quad(Om, R):
    r = R.reshape(-1, 9)
    return ((r @ Om) * r).sum(axis=1)


def minimise(Om, seed=0x5EED, n_starts=N_STARTS, max_iter=200):
    """All local minima reached from the seeded starts: (R [n_starts, 3, 3], E [n_starts])."""
    R = _random_rotations(seed, n_starts)
    E = _quad(Om, R)
    lam = np.full(n_starts, 1e-3)
    live = np.ones(n_starts, dtype=bool)
    for _ in range(max_iter):
        r = R.reshape(-1, 9)
        J = np.einsum("kab,nbc->nack", _GEN, R).reshape(-1, 9, 3)          # d vec(exp(w^) R) / d w_k = vec(G_k R)
        Jt = J.transpose(0, 2, 1)
        H = Jt @ (Om @ J)
        g = (Jt @ (r @ Om)[..., None])[..., 0]
        Hd = H + lam[:, None, None] * (np.eye(3) * np.maximum(np.einsum("nii->n", H), 1e-300)[:, None, None] / 3.0)
        try:
            w = -np.linalg.solve(Hd, g[..., None])[..., 0]
        except np.linalg.LinAlgError:
            w = -np.einsum("nij,nj->ni", np.linalg.pinv(Hd), g)
        Rn = synth.rodrigues(w) @ R
        En = _quad(Om, Rn)
        acc = live & (En < E)
        stalled = np.linalg.norm(w, axis=1) < 1e-13
        R = np.where(acc[:, None, None], Rn, R); E = np.where(acc, En, E)
        lam = np.where(acc, np.maximum(lam * 0.1, 1e-12), np.minimum(lam * 10.0, 1e12))
        live &= ~(stalled | (lam >= 1e12))
        if not live.any():
            break
    U, _, Vt = np.linalg.svd(R)                                             # (drift of 200 products: back onto SO(3))
    R = U @ Vt
    return R, _quad(Om, R)


def solve(X, xn, seed=0x5EED):
    """(R, t, E) of the global minimum in front of the camera, or None."""
    X = np.asarray(X, dtype=np.float64)
    Om, P, cen = omega_p(X, xn)
    R, E = minimise(Om, seed)
    tc = np.einsum("ij,nj->ni", P, R.reshape(-1, 9))
    t = tc - np.einsum("nij,j->ni", R, cen)
    depth = (np.einsum("nij,kj->nki", R, X)[..., 2] + t[:, None, 2]).sum(axis=1)
    ok = (depth > 0) & np.isfinite(E)
    if not ok.any():
        return None
    k = int(np.argmin(np.where(ok, E, np.inf)))
    return R[k], t[k], cost(X, xn, R[k], t[k])


def true_normalised_points(X, pose):
    """x / z, y / z of the points X [n, 3] seen from pose = (rvec, tvec): what an exact unprojection of exact detections gives."""
    pc = np.asarray(X, dtype=np.float64) @ synth.rodrigues(np.asarray(pose[:3])).T + np.asarray(pose[3:])
    return pc[:, :2] / pc[:, 2:3]

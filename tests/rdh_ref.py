"""Yardstick for the radial-distortion homography (helper, not collected): an independent f64 numpy restatement of the
six-point solver (src/optimization/homography.rs:19-167) and of its score (:169-216), with the null space from an SVD
(or, to compare two routes on the CPU, from numpy's QR) and the 6 x 4 system through numpy.linalg.lstsq, plus a generator
of EXACT division-model pairs.  The kernel is compared with this, never with itself."""
import numpy as np


def system_6x8(six):
    """Rows of the 6 x 8 system: unknowns (h00 h01 h02 h10 h11 h12 | l*h02 l*h12) of  x' (H1 . p) - y' (H0 . p) = 0  with
    p = (x, y, 1 + l r^2)."""
    x, y, xp, yp = six[:, 0], six[:, 1], six[:, 2], six[:, 3]
    r2 = x * x + y * y
    return np.stack([-x * yp, -y * yp, -yp, x * xp, y * xp, xp, -r2 * yp, r2 * xp], axis=1)


def null_space(M, route="svd"):
    if route == "svd":
        return np.linalg.svd(M)[2][6:8]
    return np.linalg.qr(M.T, mode="complete")[0][:, 6:8].T


def h6(six, route="svd"):
    """(lambda, H) of six pairs [6, 4] = (x, y, x', y'), or None."""
    six = np.asarray(six, dtype=np.float64)
    n = null_space(system_6x8(six), route)
    n0, n1 = n[0], n[1]
    # v = g n0 + n1 with v6 / v2 = v7 / v5:  a g^2 + b g + c = 0
    a = n0[6] * n0[5] - n0[7] * n0[2]
    b = n0[6] * n1[5] + n1[6] * n0[5] - n0[7] * n1[2] - n1[7] * n0[2]
    c = n1[6] * n1[5] - n1[7] * n1[2]
    disc = b * b - 4.0 * a * c
    if not disc >= 0.0:
        return None
    with np.errstate(all="ignore"):
        roots = [(b - np.sqrt(disc)) / (-2.0 * a), (b + np.sqrt(disc)) / (-2.0 * a)]
        x, y, xp, yp = six[:, 0], six[:, 1], six[:, 2], six[:, 3]
        r2 = x * x + y * y
        cand = []
        for g in roots:
            v = g * n0 + n1
            l = v[6] / v[2]
            if not np.isfinite(v).all() or not np.isfinite(l):
                cand.append(None)
                continue
            w = v[0] * x + v[1] * y + v[2] * (1.0 + l * r2)
            A = np.stack([-x * xp, -y * xp, -xp * (1.0 + l * r2), (xp * xp + yp * yp) * w], axis=1)
            if not np.isfinite(A).all():
                cand.append(None)
                continue
            sol = np.linalg.lstsq(A, -w, rcond=None)[0]
            H = np.array([[v[0], v[1], v[2]], [v[3], v[4], v[5]], [sol[0], sol[1], sol[2]]])
            cand.append((l, sol[3], H))
        ok = [cd is not None and cd[0] < 0.0 and cd[1] < 0.0 for cd in cand]
        if not ok[0] and not ok[1]:
            return None
        if ok[0] and ok[1]:
            s = [abs(np.log10(cd[0] / cd[1])) for cd in cand]
            k = 0 if s[0] < s[1] else 1
        else:
            k = 0 if ok[0] else 1
    l, lp, H = cand[k]
    return -np.sqrt(l * lp), H


def score(pairs, H, lam):
    """Mean distance of evaluate_homography_lambda: the branch of alpha is chosen on the first pair and kept."""
    pairs = np.asarray(pairs, dtype=np.float64)
    H = np.asarray(H, dtype=np.float64).reshape(3, 3)
    x, y, xp, yp = pairs[:, 0], pairs[:, 1], pairs[:, 2], pairs[:, 3]
    with np.errstate(all="ignore"):
        r = H @ np.stack([x, y, 1.0 + lam * (x * x + y * y)])
        root = np.sqrt(np.maximum(-4.0 * lam * (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2], 0.0))
        alpha = np.stack([r[2] / 2.0 - root / 2.0, r[2] / 2.0 + root / 2.0])
        k = 0 if abs(xp[0] - r[0, 0] / alpha[0, 0]) < abs(xp[0] - r[0, 0] / alpha[1, 0]) else 1
        d = np.sqrt((xp - r[0] / alpha[k]) ** 2 + (yp - r[1] / alpha[k]) ** 2)
        return float(d.sum() / len(d))


def ransac(pairs, samples, route="svd"):
    """Every hypothesis of `samples` [n_hyp, 6]: lambda, H, score (+inf where there is none) and the winner's index (-1: none)."""
    pairs = np.asarray(pairs, dtype=np.float64)
    n = len(samples)
    lam = np.zeros(n); H = np.zeros((n, 9)); sc = np.full(n, np.inf)
    for i, s in enumerate(samples):
        got = h6(pairs[np.asarray(s)], route)
        if got is None:
            continue
        v = score(pairs, got[1], got[0])
        if np.isfinite(v):
            lam[i], H[i], sc[i] = got[0], got[1].ravel(), v
    best = int(np.argmin(sc)) if np.isfinite(sc).any() else -1
    return lam, H, sc, best


def exact_pairs(lam, H, n, seed=0):
    """n exact division-model pairs: distorted points in [-0.7, 0.7]^2, undistorted by x / (1 + lam r^2), mapped by H,
    re-distorted by the closed-form inverse of the division model."""
    rng = np.random.default_rng(seed)
    pd = rng.uniform(-0.7, 0.7, size=(n, 2))
    pu = pd / (1.0 + lam * (pd * pd).sum(1, keepdims=True))
    q = np.concatenate([pu, np.ones((n, 1))], axis=1) @ np.asarray(H, dtype=np.float64).reshape(3, 3).T
    qu = q[:, :2] / q[:, 2:3]
    qd = qu * (2.0 / (1.0 + np.sqrt(1.0 - 4.0 * lam * (qu * qu).sum(1, keepdims=True))))
    return np.concatenate([pd, qd], axis=1)


def frame_pairs(f0, f1):
    """Normalised pairs of the corners both frames hold, ids ascending (src/optimization/homography.rs:223-238)."""
    w, h = f0.img_w_h
    c = np.array([w / 2.0, h / 2.0]); half = max(w / 2.0, h / 2.0)
    ids = sorted(set(f0.features) & set(f1.features))
    return np.array([np.concatenate([(np.array(f0.features[i].p2d, dtype=np.float64) - c) / half,
                                     (np.array(f1.features[i].p2d, dtype=np.float64) - c) / half]) for i in ids]).reshape(-1, 4)

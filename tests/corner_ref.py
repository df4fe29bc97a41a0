"""The yardstick of the sub-pixel corner refinement: an independent numpy f64 restatement of the rule that include/ccal.h states at
ccal_refine_corners_batch, written from that text (whole-patch array arithmetic, numpy's pairwise sums: no lane mapping, no
butterfly), and the renderer of the saddle fixtures the tests share.

refine() additionally returns, per corner, the two margins the GPU tests need to tell a rounding-sized disagreement about a
DECISION from a wrong result: the smallest |e - eps| seen at a stop test and the smallest |det / (a + d)^2 - 1e-12| / 1e-12 seen at
a degenerate test.  A corner whose margins exceed 1e-7 takes the same decisions in any arithmetic that is good to 1e-9."""
import numpy as np

OK, NOT_PD, NO_CONVERGENCE, NO_RESULT = 0, 4, 5, 8          # ccal_status


def _taps(x, n):
    x0 = np.floor(x)
    ax = x - x0
    i0 = np.clip(x0, 0, n - 1).astype(np.int64)
    return i0, np.minimum(i0 + 1, n - 1), ax


def patch(img, cx, cy, h):
    """P[j + h + 1][i + h + 1] = I(cx + i, cy + j), i, j in [-h-1, h+1]; img: f64 [H][W]."""
    H, W = img.shape
    k = np.arange(-h - 1, h + 2, dtype=np.float64)
    x0, x1, ax = _taps(cx + k, W)
    y0, y1, ay = _taps(cy + k, H)
    p00, p01 = img[np.ix_(y0, x0)], img[np.ix_(y0, x1)]
    p10, p11 = img[np.ix_(y1, x0)], img[np.ix_(y1, x1)]
    top = p00 + ax[None, :] * (p01 - p00)
    bot = p10 + ax[None, :] * (p11 - p10)
    return top + ay[:, None] * (bot - top)


def refine_one(img, c0, h, max_iterations, eps):
    """One corner: (x, y, status, iterations, lambda_min, margin_e, margin_det, and at the last evaluated iterate det / (a + d)^2 and
    whether a or d is exactly 0, and the smallest
    det / (a + d)^2 over all evaluated iterates)."""
    H, W = img.shape
    k = np.arange(-h, h + 1, dtype=np.float64)
    w1 = np.exp(-(k / h) ** 2)
    w = np.outer(w1, w1)
    sum_w = w1.sum() ** 2
    ii, jj = k[None, :], k[:, None]
    c0x, c0y = float(c0[0]), float(c0[1])
    cx, cy = c0x, c0y
    lam, it = np.nan, 0
    m_e = m_det = np.inf
    ratio, axis_edge, min_ratio = np.nan, False, np.inf
    while True:
        inside = np.isfinite(cx) and np.isfinite(cy) and h + 1 <= cx <= W - 2 - h and h + 1 <= cy <= H - 2 - h
        if not inside:
            return c0x, c0y, NO_RESULT, it, lam, m_e, m_det, float(ratio), axis_edge, min_ratio
        P = patch(img, cx, cy, h)
        gx = P[1:-1, 2:] - P[1:-1, :-2]
        gy = P[2:, 1:-1] - P[:-2, 1:-1]
        a = float((w * gx * gx).sum()); b = float((w * gx * gy).sum()); d = float((w * gy * gy).sum())
        u = float((w * (gx * gx * ii + gx * gy * jj)).sum()); v = float((w * (gx * gy * ii + gy * gy * jj)).sum())
        det = a * d - b * b
        axis_edge = min(a, d) == 0.0
        lam = ((a + d) - np.sqrt((a - d) ** 2 + 4.0 * b * b)) / (2.0 * sum_w)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.float64(det) / np.float64((a + d) ** 2)
        if np.isfinite(ratio):
            min_ratio = min(min_ratio, float(ratio))
        if np.isfinite(ratio):                       # a + d == 0: every sum is exactly 0, nothing to round
            m_det = min(m_det, abs(ratio - 1e-12) / 1e-12)
        if not det > 1e-12 * (a + d) ** 2:
            return c0x, c0y, NOT_PD, it, lam, m_e, m_det, float(ratio), axis_edge, min_ratio
        dx, dy = (d * u - b * v) / det, (a * v - b * u) / det
        cx, cy = cx + dx, cy + dy
        it += 1
        e = np.sqrt(dx * dx + dy * dy)
        m_e = min(m_e, abs(e - eps))
        if e <= eps:
            status = OK
            break
        if it >= max_iterations:
            status = NO_CONVERGENCE
            break
    if abs(cx - c0x) > h or abs(cy - c0y) > h:
        return c0x, c0y, NO_RESULT, it, lam, m_e, m_det, float(ratio), axis_edge, min_ratio
    return cx, cy, status, it, lam, m_e, m_det, float(ratio), axis_edge, min_ratio


def refine(img, xy, h, max_iterations, eps):
    """All corners [n, 2] of one image (any integer dtype, [H][W]): a dict of arrays xy [n, 2], status, iters, lam, margin_e,
    margin_det, ratio (det / (a + d)^2 at the last evaluated iterate: lambda_min is (a + d) (1 - sqrt(1 - 4 ratio)) / 2 over the
    weights' sum, so rounding in the sums reaches it magnified by about 1 / ratio; NaN: nothing evaluated, or a + d = 0) and
    axis_edge (a or d exactly 0 there: one gradient component vanishes in every pixel, and lambda_min is exactly 0)."""
    f = np.asarray(img).astype(np.float64)
    rows = [refine_one(f, c, h, max_iterations, eps) for c in np.asarray(xy, dtype=np.float64).reshape(-1, 2)]
    col = lambda i, dt=np.float64: np.array([r[i] for r in rows], dtype=dt)      # noqa: E731
    return {"xy": np.stack([col(0), col(1)], axis=1) if rows else np.zeros((0, 2)), "status": col(2, np.int32),
            "iters": col(3, np.int32), "lam": col(4), "margin_e": col(5), "margin_det": col(6), "ratio": col(7), "axis_edge": col(8, bool), "min_ratio": col(9)}


def lambda_well_conditioned(r):
    """Per corner of a refine() result: lambda_min is exactly 0 or NaN in any arithmetic (nothing evaluated, a flat patch, an
    axis-parallel edge), or det / (a + d)^2 >= 1e-5 at EVERY iterate the corner evaluated - sums that agree to 1e-15 relative (961
    terms at most, f64) then give steps and a lambda_min that agree to 1e-10.  (Measured on an MI355X: a start whose 3 x 3 window
    wandered for 22 iterations along a patch border at ratios of 6e-5 and below returned a lambda_min 3e-6 off the yardstick's.)  In between lie rank-deficient patches whose det is rounding noise (a window that
    holds a single gradient pixel): there no two orders of summation agree on lambda_min, and a fixture must not contain one."""
    with np.errstate(invalid="ignore"):
        return np.isnan(r["lam"]) | (r["axis_edge"] & (r["iters"] == 0)) | (r["min_ratio"] >= 1e-5)


# ---- fixtures -----------------------------------------------------------------------------------------------------------------
def render(width, height, centres, seed, dtype=np.uint8, sigma=1.2, amplitude=90.0, radius=14):
    """A grey image (level 128) with one saddle patch per centre: over the pixels within `radius` of the rounded centre,
    128 + s A tanh(n1 . (p - c) / sigma) tanh(n2 . (p - c) / sigma), the two edge directions within +-0.4 rad of the axes, s = +-1,
    all from the seed; rounded to uint8, or scaled by 257 and rounded to uint16.  The true saddle of patch k is centres[k]."""
    rng = np.random.default_rng(seed)
    img = np.full((height, width), 128.0)
    for cx, cy in np.asarray(centres, dtype=np.float64).reshape(-1, 2):
        t1, t2 = rng.uniform(-0.4, 0.4, 2)
        s = 1.0 if rng.random() < 0.5 else -1.0
        n1, n2 = (np.cos(t1), np.sin(t1)), (-np.sin(t2), np.cos(t2))
        rx, ry = int(round(cx)), int(round(cy))
        xs = np.arange(max(rx - radius, 0), min(rx + radius, width - 1) + 1)
        ys = np.arange(max(ry - radius, 0), min(ry + radius, height - 1) + 1)
        dx, dy = xs[None, :] - cx, ys[:, None] - cy
        img[np.ix_(ys, xs)] = 128.0 + s * amplitude * np.tanh((n1[0] * dx + n1[1] * dy) / sigma) * np.tanh((n2[0] * dx + n2[1] * dy) / sigma)
    if dtype == np.uint16:
        return np.rint(img * 257.0).astype(np.uint16)
    return np.rint(img).astype(np.uint8)


def grid_fixture(seed, n_side=5, first=16, spacing=32, radius=14, start_off=1.5, dtype=np.uint8, blank=(), sigma=1.2):
    """n_side x n_side grid positions, each jittered by up to half a pixel, in the smallest image that holds them; a saddle is
    rendered at every position but those listed in `blank` (the image stays flat there); one start per position up to start_off px
    away from it: (image, positions [n, 2] - the true saddles -, starts [n, 2])."""
    rng = np.random.default_rng(seed)
    g = first + spacing * np.arange(n_side, dtype=np.float64)
    centres = np.stack(np.meshgrid(g, g), axis=-1).reshape(-1, 2) + rng.uniform(-0.5, 0.5, (n_side * n_side, 2))
    r, phi = start_off * np.sqrt(rng.random(len(centres))), rng.uniform(0.0, 2.0 * np.pi, len(centres))
    starts = centres + np.stack([r * np.cos(phi), r * np.sin(phi)], axis=1)
    size = int(2 * first + spacing * (n_side - 1))
    drawn = np.delete(centres, list(blank), axis=0)
    return render(size, size, drawn, seed + 1, dtype=dtype, sigma=sigma, radius=radius), centres, starts


def drift_fixture():
    """h = 2 against starts 2.5 px from the saddle: (image, centres, starts)."""
    img, centres, _ = grid_fixture(105)
    phi = np.random.default_rng(5).uniform(0.0, 2.0 * np.pi, len(centres))
    return img, centres, centres + 2.5 * np.stack([np.cos(phi), np.sin(phi)], axis=1)


def rule_starts(width, height, h):
    """The starts of the status rules: exactly h + 1 from each border (inside), one ulp nearer (outside), not finite, far out."""
    lo, hx, hy, mid = h + 1.0, width - 2.0 - h, height - 2.0 - h, 0.5 * min(width, height)
    return np.array([[lo, mid], [mid, lo], [hx, mid], [mid, hy],
                     [np.nextafter(lo, 0.0), mid], [mid, np.nextafter(lo, 0.0)], [np.nextafter(hx, np.inf), mid],
                     [mid, np.nextafter(hy, np.inf)], [np.nan, mid], [mid, np.nan], [np.inf, mid], [mid, -np.inf],
                     [-5.0, 3.0], [1e300, 2.0]])


PARITY_HALF_WINS = (1, 3, 4, 15)          # 9 and 49 window pixels (under one pass of 64 lanes), 81 (a partial second), 961 (15 and 1 lane)


def parity_cases():
    """The images and starts of the GPU parity tests, {name: (image, starts [n, 2], h)}: for uint8 and uint16 and every h of
    PARITY_HALF_WINS a 160 x 160 grid of saddles with positions left flat, a start near every position, and the starts of rule_starts() that are
    not inside (the four on the border look at the rim of a patch; tests/test_gpu_corners.py::test_status_rules runs them).  A 3 x 3 window (h = 1)
    follows a saddle blurred by sigma = 1.2 px poorly, so its saddles are sharper (0.6): most of its starts end without convergence,
    at positions the parity tests compare all the same."""
    out = {}
    for di, dtype in enumerate((np.uint8, np.uint16)):
        for h in PARITY_HALF_WINS:
            seed = 200 + 40 * di + h
            if h == 15:
                img, _, starts = grid_fixture(seed, 3, 32, 48, 22, 1.5, dtype, blank=(4,))
            else:
                img, _, starts = grid_fixture(seed, 5, 16, 32, 14, min(1.5, 0.5 * h), dtype, blank=(7, 18), sigma=0.6 if h == 1 else 1.2)
            out[f"{np.dtype(dtype).name}-h{h}"] = (img, np.concatenate([starts, rule_starts(img.shape[1], img.shape[0], h)[4:]]), h)
    return out


BATCH_COUNTS = (0, 1, 63, 64, 65)         # corners per image of the batch-shape case: none, one, and around a workgroup multiple
BATCH_W, BATCH_H, BATCH_HALF_WIN = 67, 45, 3


def batch_fixture(seed=305, dtype=np.uint8):
    """Five 67 x 45 images with two saddles each and BATCH_COUNTS starts: half of them near a saddle, half anywhere in a box that
    overhangs the image by 3 px: (images [5][45][67], list of starts)."""
    rng = np.random.default_rng(seed)
    imgs, xy = [], []
    for k, n in enumerate(BATCH_COUNTS):
        centres = np.array([[20.0, 22.0], [46.0, 22.0]]) + rng.uniform(-0.5, 0.5, (2, 2))
        imgs.append(render(BATCH_W, BATCH_H, centres, seed + 1 + k, dtype=dtype, radius=9))
        near = centres[rng.integers(0, 2, n)] + rng.uniform(-1.2, 1.2, (n, 2))
        anywhere = np.stack([rng.uniform(-3.0, BATCH_W + 2.0, n), rng.uniform(-3.0, BATCH_H + 2.0, n)], axis=1)
        xy.append(np.where((rng.random(n) < 0.5)[:, None], near, anywhere))
    return np.stack(imgs), xy


# the truth test's fixture per half_win, grid_fixture(TRUTH_SEEDS[h]): 25 saddles in 160 x 160 (tests/test_corners_cpu.py; the GPU
# end-to-end test holds api.refine_corners to the same bound)
TRUTH_SEEDS = {2: 101, 3: 102, 5: 103, 7: 104}
# The worst distance (px) from the true saddle that refine() (eps 1e-3, 30 iterations) measured on grid_fixture(TRUTH_SEEDS[h]), and
# the bound the tests hold results to: 1.5 x that - the quantisation of the image is the only noise and the seeds are fixed.
TRUTH_WORST = {2: 0.07212, 3: 0.04133, 5: 0.03025, 7: 0.02663}
TRUTH_BOUND = {h: 1.5 * v for h, v in TRUTH_WORST.items()}
